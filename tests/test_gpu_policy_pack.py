"""GPU: the device repack of a policy's weights (k_policy_pack behind `MlpPolicy.load_weights_device`) against the host
packer it shares its arithmetic with (mse_policy_pack_host, which tests/test_policy_pack_cpu.py holds against an
independent restatement): the image byte for byte at every shape and weight set of that file, the f16 range flag and
what it does to an auto and to a pinned policy, bit-equal forwards and rollouts from a host-loaded and a device-loaded
policy, the stream ordering, and the weights read back from the handle."""
import ctypes as C

import numpy as np
import pytest

from tests import policy_pack_reference as R

pytestmark = pytest.mark.gpu


def _policy(D, A, flat, precision="auto"):
    import marl_sortingenv_amd as M
    from marl_sortingenv_amd.policy import SB3_KEYS, _shapes

    parts = [p.reshape(s) for p, s in zip(R.split(flat, D, A), _shapes(D, A))]
    return M.MlpPolicy(D, A, dict(zip(SB3_KEYS, parts)), device=0, precision=precision)


def _image(pol):
    img = np.full(R.IMAGE_FLOATS, np.nan, dtype=np.float32)
    assert pol.L.mse_policy_read_image(pol._h, C.c_void_p(img.ctypes.data)) == 0
    return img.view(np.uint32)


def _host_image(pol, flat):
    img = np.empty(R.IMAGE_FLOATS, dtype=np.float32)
    ok = C.c_int32(-1)
    assert pol.L.mse_policy_pack_host(pol.obs_dim, pol.n_actions, C.c_void_p(flat.ctypes.data), C.c_void_p(img.ctypes.data), C.byref(ok)) == 0
    return img.view(np.uint32), bool(ok.value)


@pytest.mark.parametrize("D,A", R.SHAPES)
def test_device_image_equals_the_host_image(D, A):
    import torch

    start = R.sb3_scale(D, A, 11)
    dev_pol, host_pol = _policy(D, A, start), _policy(D, A, start)
    assert np.array_equal(_image(dev_pol), _host_image(dev_pol, start)[0])  # mse_policy_create, through the same walk
    # "above" in the middle: an auto policy goes to f32 on overflow and comes back when the weights fit again
    for name in ("sb3", "tiny", "above", "below"):
        flat, expect_ok = R.weight_sets(D, A)[name]
        want, ok = _host_image(dev_pol, flat)
        assert ok == expect_ok
        dev_pol.load_weights_device(torch.from_numpy(flat).cuda())
        host_pol.load_weights(flat)
        cells = R.compared_cells(ok)
        got = _image(dev_pol)
        bad = np.flatnonzero(got[cells] != want[cells])
        assert bad.size == 0, (name, bad[:8], got[bad[:8]], want[bad[:8]])
        assert np.array_equal(_image(host_pol)[cells], want[cells])
        assert dev_pol.precision == host_pol.precision == ("f16x3" if ok else "f32"), name
        assert dev_pol.L.mse_policy_precision(dev_pol._h) == (2 if ok else 1)
        assert np.array_equal(dev_pol.flat_weights().view(np.uint32), flat.view(np.uint32))
        assert np.array_equal(host_pol.flat_weights().view(np.uint32), flat.view(np.uint32))


def test_an_f32_policy_keeps_its_form_and_a_pinned_f16_policy_refuses_overflow():
    import torch

    import marl_sortingenv_amd as M

    D, A = 29, 22
    start = R.sb3_scale(D, A, 11)
    above, below = R.weight_sets(D, A)["above"][0], R.weight_sets(D, A)["below"][0]
    exact = _policy(D, A, start, precision="f32")
    exact.load_weights_device(torch.from_numpy(below).cuda())
    assert exact.precision == "f32" and np.array_equal(_image(exact), _host_image(exact, below)[0])
    pinned = _policy(D, A, start, precision="f16x3")
    before = _image(pinned).copy()
    with pytest.raises(M.MseError) as err:
        pinned.load_weights_device(torch.from_numpy(above).cuda())
    assert err.value.status == -2
    assert np.array_equal(_image(pinned), before)  # image unchanged, bit for bit
    assert pinned.precision == "f16x3" and np.array_equal(pinned.flat_weights().view(np.uint32), start.view(np.uint32))
    # without the sync nothing raises until it is asked for; a later good load clears the refusal
    pinned.load_weights_device(torch.from_numpy(above).cuda(), sync=False)
    with pytest.raises(M.MseError):
        pinned.sync()
    pinned.load_weights_device(torch.from_numpy(below).cuda())
    assert np.array_equal(_image(pinned), _host_image(pinned, below)[0]) and pinned.sync() == "f16x3"


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_forward_is_bit_equal_between_a_host_loaded_and_a_device_loaded_policy(precision):
    import torch

    D, A, n = 29, 22, 65  # two tiles and a tail
    start, new = R.sb3_scale(D, A, 11), R.sb3_scale(D, A, 12)
    host_pol, dev_pol = _policy(D, A, start, precision), _policy(D, A, start, precision)
    host_pol.load_weights(new)
    dev_pol.load_weights_device(torch.from_numpy(new).cuda())
    g = torch.Generator().manual_seed(3)
    obs = torch.randn(n, D, generator=g).cuda()
    mask = (torch.rand(n, A, generator=g) < 0.7).to(torch.uint8)
    mask[:, 0] = 1
    a = host_pol.forward(obs, mask.cuda(), seed=9, t=4, want_logits=True)
    b = dev_pol.forward(obs, mask.cuda(), seed=9, t=4, want_logits=True)
    for key in ("action", "logp", "value", "logits"):
        assert torch.equal(a[key].view(torch.int32), b[key].view(torch.int32)), key
    fresh = _policy(D, A, new, precision).forward(obs, mask.cuda(), seed=9, t=4, want_logits=True)
    assert torch.equal(fresh["logits"].view(torch.int32), b["logits"].view(torch.int32))
    assert not torch.equal(_policy(D, A, start, precision).forward(obs, mask.cuda(), seed=9, t=4, want_logits=True)["logits"], b["logits"])


@pytest.mark.parametrize("kind", ["mono", "press"])
def test_fused_rollout_is_bit_equal_between_the_two(kind):
    import torch

    import marl_sortingenv_amd as M

    D, A = M.OBS_DIM[kind], M.NUM_ACTIONS[kind]
    start, new = R.sb3_scale(D, A, 21), R.sb3_scale(D, A, 22)
    sort_start, sort_new = R.sb3_scale(13, 2, 23), R.sb3_scale(13, 2, 24)
    out = []
    for device_loaded in (False, True):
        pol = _policy(D, A, start)
        sort_pol = _policy(13, 2, sort_start) if kind == "press" else None
        for p, w in ((pol, new), (sort_pol, sort_new)):
            if p is None:
                continue
            if device_loaded:
                p.load_weights_device(torch.from_numpy(w).cuda())
            else:
                p.load_weights(w)
        env = M.BatchedSortingEnv(kind=kind, num_envs=256, device=0, base_seed=21, max_steps=5, noise_sorting=0.05, balesize=200,
                                  auto_reset=True)
        col = M.FusedPolicyRollout(env, pol, 4, seed=22, sort_policy=sort_pol)
        out.append({k: v.clone() for k, v in col.collect().items()})
    torch.cuda.synchronize()
    assert set(out[0]) == set(out[1]) and len(out[0]) == 9
    for k in out[0]:
        same = torch.equal(out[0][k].view(torch.uint8) if out[0][k].dtype == torch.uint8 else out[0][k].view(torch.int32),
                           out[1][k].view(torch.uint8) if out[1][k].dtype == torch.uint8 else out[1][k].view(torch.int32))
        assert same, (kind, k)


def test_a_repack_enqueued_behind_an_adam_step_is_seen_by_the_next_forward():
    """no synchronisation between the three: the stream orders them"""
    import torch

    import marl_sortingenv_amd as M

    D, A, n = 29, 22, 65
    start = R.sb3_scale(D, A, 11)
    pol = _policy(D, A, start)
    learner = M.PPOLearner(pol, learning_rate=1e-2)
    g = torch.Generator().manual_seed(5)
    obs = torch.randn(n, D, generator=g).cuda()
    learner.grad.copy_(torch.randn(learner.n_weights, generator=g).cuda())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        learner.adam_step()
        pol.load_weights_device(learner.weights, sync=False)
        got = pol.forward(obs, None, deterministic=True, want_logits=True)
    side.synchronize()
    assert pol.sync() == "f16x3"
    stepped = learner.weights.cpu().numpy()
    assert not np.array_equal(stepped, start)
    want = _policy(D, A, stepped).forward(obs, None, deterministic=True, want_logits=True)
    torch.cuda.synchronize()
    for key in ("action", "value", "logits"):
        assert torch.equal(got[key].view(torch.int32), want[key].view(torch.int32)), key
    assert np.array_equal(_image(pol), _host_image(pol, stepped)[0])


def test_the_policy_returns_the_weights_that_were_loaded_even_after_the_source_is_overwritten():
    import torch

    from marl_sortingenv_amd.policy import SB3_KEYS

    D, A = 16, 11
    pol = _policy(D, A, R.sb3_scale(D, A, 11))
    new = R.sb3_scale(D, A, 12)
    src = torch.from_numpy(new).cuda()
    pol.load_weights_device(src)
    src.fill_(7.0)  # as a later Adam step overwrites the learner's master vector
    torch.cuda.synchronize()
    assert np.array_equal(pol.flat_weights().view(np.uint32), new.view(np.uint32))
    sd = pol.state_dict()
    assert list(sd) == SB3_KEYS
    for t, part in zip(sd.values(), R.split(new, D, A)):
        assert tuple(t.shape)[-1] == part.shape[-1] and np.array_equal(t.numpy().ravel(), part.ravel())
    assert np.array_equal(np.concatenate([pol.weights[k].ravel() for k in SB3_KEYS]), new)
    with pytest.raises(ValueError):
        pol.load_weights_device(torch.from_numpy(new))  # a host tensor
    with pytest.raises(ValueError):
        pol.load_weights_device(src[:-1])
