"""GPU: the two decisions `PPOLearner.update()` no longer takes on the host.

weight_sync="device" (one repack launch instead of the copy down, the host repack and the blocking copy up) against
weight_sync="host": twin learners and policies on one rollout, everything bit for bit.

target_kl (SB3's early stop, decided by a flag on the device) against a loop written out by hand over the UNGATED
`loss_grad` / `adam_step` that reads approx_kl on the host after every minibatch and applies SB3's rule: no optimiser
step for the minibatch whose approx_kl exceeds 1.5 * target_kl and no minibatch after it.  The threshold comes from an
ungated dry run of the same update, so the stop is known to fall strictly inside it.

One mono rollout of 64 envs x 4 steps = 256 rows, n_epochs=2, batch_size=100: minibatches of 100, 100 and 56 rows, six per
update."""
import ctypes as C

import numpy as np
import pytest

from tests import policy_pack_reference as PR
from tests.ppo_checks import DIMS, HP, make_policy

pytestmark = pytest.mark.gpu

N, K, EPOCHS, BS, SEED = 64, 4, 2, 100, 5
TOTAL = N * K
PER_EPOCH = -(-TOTAL // BS)
M_UPDATE = EPOCHS * PER_EPOCH  # minibatches per update
LR_RISING = 3e-4               # small enough that approx_kl keeps rising over the Adam steps of an update


def _setup(lr=1e-3, **kw):
    import marl_sortingenv_amd as M

    pol, _ = make_policy(*DIMS["mono"], 31)
    env = M.BatchedSortingEnv(kind="mono", num_envs=N, device=0, base_seed=21, max_steps=5, noise_sorting=0.05, balesize=200,
                              auto_reset=True)
    col = M.FusedPolicyRollout(env, pol, K, seed=22)
    return pol, col, M.PPOLearner(pol, learning_rate=lr, n_epochs=EPOCHS, batch_size=BS, seed=SEED, **HP, **kw)


def _rollout():
    _, col, _ = _setup()
    return {k: v.clone() for k, v in col.collect().items()}


def _bits(t):
    import torch

    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    import torch

    return torch.equal(_bits(a), _bits(b))


def _image(pol):
    img = np.empty(PR.IMAGE_FLOATS, dtype=np.float32)
    assert pol.L.mse_policy_read_image(pol._h, C.c_void_p(img.ctypes.data)) == 0
    return img.view(np.uint32)


def _host_image(pol, flat):
    flat = np.ascontiguousarray(flat, dtype=np.float32)
    img = np.empty(PR.IMAGE_FLOATS, dtype=np.float32)
    ok = C.c_int32(-1)
    assert pol.L.mse_policy_pack_host(pol.obs_dim, pol.n_actions, C.c_void_p(flat.ctypes.data), C.c_void_p(img.ctypes.data), C.byref(ok)) == 0
    return img.view(np.uint32)


def _assert_same_learner(a, b, label):
    for name in ("weights", "m", "v"):
        assert _same_bits(getattr(a, name), getattr(b, name)), (label, name)
    assert a.step == b.step, label


def _assert_policy_holds(pol, learner, label):
    flat = learner.weights.cpu().numpy()
    assert np.array_equal(_image(pol), _host_image(pol, flat)), label
    assert np.array_equal(pol.flat_weights().view(np.uint32), flat.view(np.uint32)), label


# ---- weight_sync ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shuffle", ["cpu", "device"])
@pytest.mark.parametrize("host_path_barred", [False, True])
def test_device_weight_sync_equals_host_weight_sync(shuffle, host_path_barred, monkeypatch):
    import torch

    data = _rollout()
    hpol, _, host = _setup(shuffle=shuffle)
    dpol, _, dev = _setup(shuffle=shuffle, weight_sync="device")
    assert host.weight_sync == "host" and dev.weight_sync == "device"
    if host_path_barred:
        def barred(*a, **k):
            raise AssertionError("weight_sync='device' must not go through MlpPolicy.load_weights")

        monkeypatch.setattr(dpol, "load_weights", barred)
    for u in range(2):
        out_h, out_d = host.update(data), dev.update(data)
        torch.cuda.synchronize()
        _assert_same_learner(host, dev, (shuffle, u))
        assert _same_bits(out_h["stats"], out_d["stats"]) and out_h["mean"] == out_d["mean"]
        assert "stopped" not in out_d and out_d["stats"].shape == (M_UPDATE, 8)
        assert np.array_equal(_image(hpol), _image(dpol)), (shuffle, u)
        assert hpol.precision == dpol.precision == "f16x3"
        _assert_policy_holds(dpol, dev, (shuffle, u))
    assert dev.step == 2 * M_UPDATE


def test_restore_best_under_device_sync_restores_the_image_of_the_best_weights(monkeypatch):
    import torch

    data = _rollout()
    pol, _, learner = _setup(weight_sync="device")
    with pytest.raises(RuntimeError):
        learner.restore_best()
    learner.update(data)
    learner.best_weights = learner.weights.clone()
    best = learner.best_weights.cpu().numpy()
    learner.update(data)
    assert not np.array_equal(pol.flat_weights(), best)
    monkeypatch.setattr(pol, "load_weights", None)  # calling it would raise
    learner.restore_best()
    torch.cuda.synchronize()
    assert np.array_equal(learner.weights.cpu().numpy().view(np.uint32), best.view(np.uint32))
    assert np.array_equal(_image(pol), _host_image(pol, best))
    assert np.array_equal(pol.flat_weights().view(np.uint32), best.view(np.uint32))


def test_learn_with_both_options_equals_the_loop_written_out_by_hand():
    import torch

    opts = dict(lr=LR_RISING, shuffle="device", target_kl=0.01)
    _, col_a, a = _setup(weight_sync="device", **opts)
    _, col_b, b = _setup(weight_sync="device", **opts)
    _, col_c, c = _setup(weight_sync="host", **opts)
    history = a.learn(col_a, iterations=3)
    by_hand = []
    for _ in range(3):
        data = col_b.collect()
        out = b.update(data)
        by_hand.append(dict(out["mean"], reward=float(data["rewards"].mean()), stopped=out["stopped"],
                            minibatches_run=out["minibatches_run"]))
    history_c = c.learn(col_c, iterations=3)
    torch.cuda.synchronize()
    assert history == by_hand and history == history_c
    _assert_same_learner(a, b, "hand loop")
    _assert_same_learner(a, c, "host twin")
    _assert_policy_holds(a.policy, a, "learn")
    assert a.epochs_done == 3 * EPOCHS  # the epochs enqueued, stopped or not


# ---- target_kl ------------------------------------------------------------------------------------------------------------
def _permutations(hand, generator):
    """the row orders of one update, as update() draws them: all n_epochs of them, whether or not the update stops"""
    import torch

    if hand.shuffle == "device":
        perms = [hand.permutation(TOTAL, hand.epochs_done + e) for e in range(EPOCHS)]
        hand.epochs_done += EPOCHS
        return perms
    return [torch.randperm(TOTAL, generator=generator) for _ in range(EPOCHS)]


def _update_by_hand(hand, data, generator, target_kl):
    """SB3's PPO.train with target_kl from the ungated public pieces, one host read per minibatch.  Returns (stats with
    NaN in the rows that did not run, minibatches run, stopped)."""
    import torch

    import marl_sortingenv_amd as M

    M.compute_gae(data, hand.gamma, hand.gae_lambda)
    stats = torch.full((M_UPDATE, 8), float("nan"), device="cuda")
    i = 0
    for perm in _permutations(hand, generator):
        rows = perm.cuda()
        for start in range(0, TOTAL, BS):
            mb = rows[start:start + BS]
            hand.loss_grad(data, mb, mb.numel(), stats[i])
            i += 1
            approx_kl = float(stats[i - 1, 4].item())  # a float32 mean against a Python float, as SB3 compares them
            if target_kl is not None and approx_kl > 1.5 * target_kl:
                return stats, i, True
            hand.adam_step()
    return stats, i, False


@pytest.mark.parametrize("shuffle", ["cpu", "device"])
@pytest.mark.parametrize("weight_sync", ["host", "device"])
def test_target_kl_stops_where_the_hand_loop_stops(shuffle, weight_sync):
    import torch

    data = _rollout()
    # the threshold, from an ungated dry run of the same update
    _, _, dry = _setup(lr=LR_RISING, shuffle=shuffle)
    kl = dry.update(data)["stats"][:, 4].cpu().tolist()
    print("approx_kl of the ungated update:", kl)
    rising = [j for j in range(1, M_UPDATE - 1) if kl[j] > max(kl[:j])]
    assert rising, "approx_kl never rises above its past inside the update: no stop to test"
    j = rising[-1]
    assert 1 <= j <= M_UPDATE - 2
    threshold = 0.5 * (max(kl[:j]) + kl[j])
    target_kl = threshold / 1.5
    assert max(kl[:j]) < 1.5 * target_kl < kl[j]

    pol, _, gated = _setup(lr=LR_RISING, shuffle=shuffle, weight_sync=weight_sync, target_kl=target_kl)
    _, _, hand = _setup(lr=LR_RISING, shuffle=shuffle)
    generator = torch.Generator().manual_seed(SEED)
    out = gated.update(data)
    want_stats, want_run, want_stopped = _update_by_hand(hand, data, generator, target_kl)
    torch.cuda.synchronize()
    print("stopped at minibatch", out["minibatches_run"] - 1, "expected", j)
    assert want_stopped and want_run == j + 1  # the yardstick itself stops where the dry run says
    assert out["stopped"] is True and out["minibatches_run"] == j + 1
    _assert_same_learner(gated, hand, "first update")
    assert gated.step == j  # Adam steps taken: the stopping minibatch took none
    assert _same_bits(out["stats"][:j + 1], want_stats[:j + 1])
    assert torch.count_nonzero(_bits(out["stats"][j + 1:])) == 0  # update() hands out zeros; nothing wrote there
    assert out["mean"] == dict(zip(("loss", "policy_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction", "adv_mean",
                                    "adv_std"), out["stats"][:j + 1].cpu().mean(dim=0).tolist()))
    _assert_policy_holds(pol, gated, "first update")
    assert gated.epochs_done == (EPOCHS if shuffle == "device" else 0)
    # a second update continued on both sides
    out2 = gated.update(data)
    want_stats2, want_run2, want_stopped2 = _update_by_hand(hand, data, generator, target_kl)
    torch.cuda.synchronize()
    assert (out2["stopped"], out2["minibatches_run"]) == (want_stopped2, want_run2)
    _assert_same_learner(gated, hand, "second update")
    assert _same_bits(out2["stats"][:want_run2], want_stats2[:want_run2])
    _assert_policy_holds(pol, gated, "second update")


def test_a_closed_gate_writes_nothing_and_an_open_one_changes_nothing():
    import torch

    data = _rollout()
    _, _, learner = _setup(lr=LR_RISING)
    _, _, plain = _setup(lr=LR_RISING)
    import marl_sortingenv_amd as M

    M.compute_gae(data, learner.gamma, learner.gae_lambda)
    rows = torch.randperm(TOTAL, generator=torch.Generator().manual_seed(1))[:BS].cuda()
    nan = float("nan")
    # open, and no threshold to cross (target_kl <= 0): the ungated call's bits, and the count
    control = torch.zeros(2, dtype=torch.int32, device="cuda")
    stats, want_stats = torch.full((2, 8), nan, device="cuda"), torch.full((2, 8), nan, device="cuda")
    learner.loss_grad(data, rows, BS, stats[0], control=control, target_kl=0.0)
    plain.loss_grad(data, rows, BS, want_stats[0])
    learner.adam_step(control)
    plain.adam_step()
    assert control.tolist() == [0, 1]
    assert _same_bits(stats, want_stats) and _same_bits(learner.grad, plain.grad)
    _assert_same_learner(learner, plain, "open gate")
    # a threshold below this minibatch's approx_kl (the weights have moved): statistics written, flag set, no Adam step
    before = [t.clone() for t in (learner.weights, learner.m, learner.v)]
    learner.loss_grad(data, rows, BS, stats[1], control=control, target_kl=1e-12)
    plain.loss_grad(data, rows, BS, want_stats[1])
    learner.adam_step(control)
    assert control.tolist() == [1, 2] and float(stats[1, 4]) > 1.5e-12
    assert _same_bits(stats, want_stats) and _same_bits(learner.grad, plain.grad)
    # closed: nothing is written, whatever the threshold
    grad = torch.full_like(learner.grad, nan)
    untouched = torch.full((8,), nan, device="cuda")
    learner.loss_grad(data, rows, BS, untouched, grad_out=grad, control=control, target_kl=1e9)
    learner.adam_step(control)
    torch.cuda.synchronize()
    assert control.tolist() == [1, 2]
    assert bool(torch.isnan(untouched).all()) and bool(torch.isnan(grad).all())
    for t, b in zip((learner.weights, learner.m, learner.v), before):
        assert _same_bits(t, b)


@pytest.mark.parametrize("shuffle", ["cpu", "device"])
def test_a_target_kl_that_never_trips_and_none_are_todays_update(shuffle):
    import torch

    data = _rollout()
    _, _, plain = _setup(shuffle=shuffle)
    _, _, never = _setup(shuffle=shuffle, target_kl=1e9)
    _, _, none = _setup(shuffle=shuffle, target_kl=None, weight_sync="host")
    for u in range(2):
        out_p, out_n, out_0 = plain.update(data), never.update(data), none.update(data)
        torch.cuda.synchronize()
        _assert_same_learner(plain, never, u)
        _assert_same_learner(plain, none, u)
        assert _same_bits(out_p["stats"], out_n["stats"]) and _same_bits(out_p["stats"], out_0["stats"])
        assert sorted(out_p) == sorted(out_0) == ["mean", "stats"] and out_p["mean"] == out_0["mean"]
        assert out_n["stopped"] is False and out_n["minibatches_run"] == M_UPDATE
        # the gated path forms "mean" on the host from the copied rows, today's on the device: same rows, so equal to
        # float32 rounding of a six-term mean
        for name, v in out_p["mean"].items():
            assert out_n["mean"][name] == pytest.approx(v, rel=1e-6, abs=1e-9), name
    assert plain.step == never.step == 2 * M_UPDATE
