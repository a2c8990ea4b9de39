"""GPU: the on-device PPO learner (mse_gae, mse_ppo_loss_grad, mse_ppo_adam_step, mse_policy_set_weights, PPOLearner)
against tests/ppo_reference.py - numpy float32 for GAE (bit-equal), float64 torch autograd for the loss and gradient,
float64 clip_grad_norm_ + Adam.  Tolerances: the rule written in tests/ppo_reference.py (4 x the error of torch's own
float32 CPU evaluation against float64, computed each run; nothing is taken from the kernels)."""
import numpy as np
import pytest

from tests import ppo_reference as R
from tests.ppo_checks import DIMS, HP, check_loss_grad, cpu_rows as _cpu, make_policy, random_gae_inputs

pytestmark = pytest.mark.gpu


def _policy(kind, seed, saturating=False, precision="auto"):
    return make_policy(*DIMS[kind], seed, saturating=saturating, precision=precision)


def _rollout(kind, n, K, seed, policy, max_steps=5):
    import marl_sortingenv_amd as M

    env = M.BatchedSortingEnv(kind=kind, num_envs=n, device=0, base_seed=seed, max_steps=max_steps, noise_sorting=0.05,
                              balesize=200, auto_reset=True)
    col = M.FusedPolicyRollout(env, policy, K, seed=seed + 1)
    return env, col


def _gae_inputs_numpy(d):
    return [d[k].cpu().numpy() for k in ("rewards", "values", "episode_starts", "last_values", "last_dones")]


def test_gae_on_a_real_rollout_is_bit_equal_to_sb3():
    import torch

    import marl_sortingenv_amd as M

    pol, _ = _policy("mono", 3)
    env, col = _rollout("mono", 65537, 16, 5, pol, max_steps=5)
    data = col.collect()
    M.compute_gae(data, 0.99, 0.95)
    torch.cuda.synchronize()
    es = data["episode_starts"].cpu().numpy()
    assert es[1:].any(axis=0).all(), "every env ends an episode inside the rollout"
    ea, er = R.gae_numpy(*_gae_inputs_numpy(data), 0.99, 0.95)
    assert np.array_equal(data["advantages"].cpu().numpy().view(np.uint32), ea.view(np.uint32))
    assert np.array_equal(data["returns"].cpu().numpy().view(np.uint32), er.view(np.uint32))


def _check_gae(d, pairs, label):
    import marl_sortingenv_amd as M

    for gamma, lam in pairs:
        M.compute_gae(d, gamma, lam)
        ea, er = R.gae_numpy(*_gae_inputs_numpy(d), gamma, lam)
        assert np.array_equal(d["advantages"].cpu().numpy().view(np.uint32), ea.view(np.uint32)), (label, gamma, lam)
        assert np.array_equal(d["returns"].cpu().numpy().view(np.uint32), er.view(np.uint32)), (label, gamma, lam)


GAE_PAIRS = ((0.99, 0.95), (0.9, 1.0), (1.0, 0.0), (0.0, 1.0))


@pytest.mark.parametrize("n", [1, 63, 255, 256, 257, 2 ** 20 + 1])
def test_gae_on_random_inputs(n):
    _check_gae(random_gae_inputs(9, n, n), GAE_PAIRS, n)


# K = 9 with random starts is test_gae_on_random_inputs
GAE_EDGES = [(n, K, starts) for n in (1, 63, 255, 256, 257, 2 ** 20 + 1) for K in (1, 2, 9) for starts in ("random", "ones", "zeros")
             if (K, starts) != (9, "random")]


@pytest.mark.parametrize("n,K,starts", GAE_EDGES)
def test_gae_launch_edges(n, K, starts):
    _check_gae(random_gae_inputs(K, n, n, starts), GAE_PAIRS, (n, K, starts))


def test_compute_gae_converts_its_inputs_and_reuses_its_outputs():
    import torch

    import marl_sortingenv_amd as M

    K, n = 5, 257
    d = random_gae_inputs(K, n, 3)
    M.compute_gae(d, 0.99, 0.95)
    want_a, want_r = d["advantages"].clone(), d["returns"].clone()
    wide = torch.zeros((K, 2 * n), device="cuda")
    wide[:, ::2] = d["values"]
    other = {"rewards": d["rewards"].double(), "values": wide[:, ::2], "episode_starts": d["episode_starts"].bool(),
             "last_values": d["last_values"].double(), "last_dones": d["last_dones"].bool()}
    assert not other["values"].is_contiguous()
    M.compute_gae(other, 0.99, 0.95)
    assert other["advantages"].dtype == torch.float32 and other["advantages"].is_contiguous()
    assert torch.equal(other["advantages"].view(torch.int32), want_a.view(torch.int32))
    assert torch.equal(other["returns"].view(torch.int32), want_r.view(torch.int32))
    # fitting outputs already in the dict are written in place ...
    ptrs = (other["advantages"].data_ptr(), other["returns"].data_ptr())
    other["advantages"].fill_(float("nan"))
    other["returns"].fill_(float("nan"))
    M.compute_gae(other, 0.99, 0.95)
    assert (other["advantages"].data_ptr(), other["returns"].data_ptr()) == ptrs
    assert torch.equal(other["advantages"].view(torch.int32), want_a.view(torch.int32))
    assert torch.equal(other["returns"].view(torch.int32), want_r.view(torch.int32))
    # ... and ones that do not fit (shape, dtype, layout) are replaced, not written through
    stale = torch.zeros((K, n + 1), device="cuda")
    other["advantages"], other["returns"] = stale, torch.zeros((K, n), dtype=torch.float64, device="cuda")
    M.compute_gae(other, 0.99, 0.95)
    assert other["advantages"].data_ptr() != stale.data_ptr() and not bool(stale.any())
    assert other["returns"].dtype == torch.float32
    assert torch.equal(other["advantages"].view(torch.int32), want_a.view(torch.int32))
    assert torch.equal(other["returns"].view(torch.int32), want_r.view(torch.int32))


def _check_loss_grad(kind, flat, learner, data, rows_cpu, label, yardstick_rows=None):
    """tests/ppo_checks.py's check_loss_grad for one of the three env shapes -> the float64 loss"""
    return check_loss_grad(*DIMS[kind], flat, learner, data, rows_cpu, label, yardstick_rows=yardstick_rows)[0]


@pytest.mark.parametrize("saturating", [False, True])
@pytest.mark.parametrize("kind", ["sort", "press", "mono"])
def test_loss_grad_matches_float64_autograd_small(kind, saturating):
    import torch

    import marl_sortingenv_amd as M

    pol, flat = _policy(kind, 11, saturating=saturating)
    env, col = _rollout(kind, 1000, 12, 7, pol)
    data = col.collect()
    learner = M.PPOLearner(pol, **HP)
    M.compute_gae(data)
    # the policy that collected is the policy evaluated: ratio = 1 up to the f16x3 rollout arithmetic; move the old
    # log-probabilities so that both clip sides occur
    g = torch.Generator().manual_seed(3)
    data["log_probs"] = (data["log_probs"] + (torch.rand(data["log_probs"].shape, generator=g) * 0.8 - 0.4).cuda()).contiguous()
    rows = torch.randperm(12 * 1000, generator=g)[:4096]
    _check_loss_grad(kind, flat, learner, data, rows, f"{kind} sat={saturating} 4096 rows_dev")
    _check_loss_grad(kind, flat, learner, data, rows[:1], f"{kind} sat={saturating} B=1", yardstick_rows=rows[:64])
    _check_loss_grad(kind, flat, learner, data, rows[:77], f"{kind} sat={saturating} B=77")


@pytest.mark.parametrize("saturating", [False, True])
def test_loss_grad_matches_float64_autograd_full_rollout(saturating):
    import torch

    import marl_sortingenv_amd as M

    pol, flat = _policy("mono", 13, saturating=saturating)
    env, col = _rollout("mono", 65536, 16, 9, pol)
    data = col.collect()
    learner = M.PPOLearner(pol, **HP)
    M.compute_gae(data)
    g = torch.Generator().manual_seed(4)
    data["log_probs"] = (data["log_probs"] + (torch.rand(data["log_probs"].shape, generator=g) * 0.8 - 0.4).cuda()).contiguous()
    rows = torch.randperm(16 * 65536, generator=g)[:4096]
    _check_loss_grad("mono", flat, learner, data, rows, f"mono sat={saturating} 4096 of 2^20")
    _check_loss_grad("mono", flat, learner, data, None, f"mono sat={saturating} all 2^20 rows")


def _check_adam_state(learner, st64, st32, label):
    """m and v under the rule of the weights: 4 x the error of torch's float32 Adam, relative to the max-norm"""
    for name, got, r64, r32 in (("m", learner.m, st64[0], st32[0]), ("v", learner.v, st64[1], st32[1])):
        scale = float(r64.abs().max())
        e32 = float((r32.double() - r64).abs().max()) / scale
        err = float((got.cpu().double() - r64).abs().max()) / scale
        assert err <= 4 * e32, (label, name, err, e32)


def test_adam_step_matches_torch_float64():
    import torch

    import marl_sortingenv_amd as M

    pol, flat = _policy("mono", 17)
    W = flat.numel()
    for max_norm, gscale in ((0.5, 5.0), (0.5, 1e-3), (0.0, 1.0)):  # norm above / below max_grad_norm, no clipping
        learner = M.PPOLearner(pol, learning_rate=3e-4, max_grad_norm=max_norm)
        g = torch.Generator().manual_seed(5)
        grads = [torch.randn(W, generator=g) * gscale / W ** 0.5 for _ in range(20)]
        st64, st32 = [], []
        ref64, norms64 = R.adam_reference(flat, grads, 3e-4, 1e-5, max_norm, torch.float64, states=st64)
        ref32, _ = R.adam_reference(flat, grads, 3e-4, 1e-5, max_norm, torch.float32, states=st32)
        for k, gk in enumerate(grads):
            learner.grad.copy_(gk)
            learner.adam_step()
            torch.cuda.synchronize()
            got = learner.weights.cpu().double()
            # the update w - w0 is what the optimiser computes; yardstick as for the gradient
            upd64 = ref64[k] - flat.double()
            scale = float(upd64.abs().max())
            e32 = float((ref32[k].double() - ref64[k]).abs().max()) / scale
            err = float((got - ref64[k]).abs().max()) / scale
            assert err <= 4 * e32, (max_norm, gscale, k, err, e32)
            _check_adam_state(learner, st64[k], st32[k], (max_norm, gscale, k))
            assert abs(float(learner.grad_norm.cpu()) - norms64[k]) <= 4 * np.finfo(np.float32).eps * norms64[k]
        assert (norms64[0] > max_norm) == (gscale == 5.0) or max_norm == 0.0


@pytest.mark.parametrize("D,A", [DIMS["sort"], (32, 32)])
def test_adam_step_other_sizes_and_a_late_start(D, A):
    """n_weights other than mono's; a run that starts at step 10 000 (bias corrections ~ 1) from non-zero m and v."""
    import torch

    import marl_sortingenv_amd as M

    pol, flat = make_policy(D, A, 61)
    W = flat.numel()
    g = torch.Generator().manual_seed(6)
    for start, gscale in ((0, 5.0), (10_000, 5.0), (10_000, 1e-3)):
        learner = M.PPOLearner(pol, learning_rate=3e-4, max_grad_norm=0.5)
        m0 = v0 = None
        if start:
            m0 = (torch.randn(W, generator=g) * gscale / W ** 0.5 * 0.1).float()
            v0 = ((torch.randn(W, generator=g) * gscale / W ** 0.5 * 0.1) ** 2).float()
            learner.step = start
            learner.m.copy_(m0)
            learner.v.copy_(v0)
        grads = [torch.randn(W, generator=g) * gscale / W ** 0.5 for _ in range(8)]
        st64, st32 = [], []
        ref64, norms64 = R.adam_reference(flat, grads, 3e-4, 1e-5, 0.5, torch.float64, start, m0, v0, st64)
        ref32, _ = R.adam_reference(flat, grads, 3e-4, 1e-5, 0.5, torch.float32, start, m0, v0, st32)
        for k, gk in enumerate(grads):
            learner.grad.copy_(gk)
            learner.adam_step()
            torch.cuda.synchronize()
            upd64 = ref64[k] - flat.double()
            scale = float(upd64.abs().max())
            e32 = float((ref32[k].double() - ref64[k]).abs().max()) / scale
            err = float((learner.weights.cpu().double() - ref64[k]).abs().max()) / scale
            assert err <= 4 * e32, (start, gscale, k, err, e32)
            _check_adam_state(learner, st64[k], st32[k], (start, gscale, k))
            assert abs(float(learner.grad_norm.cpu()) - norms64[k]) <= 4 * np.finfo(np.float32).eps * norms64[k]
        assert learner.step == start + len(grads)


def test_adam_step_with_a_zero_gradient_changes_nothing():
    import torch

    import marl_sortingenv_amd as M

    pol, flat = _policy("mono", 67)
    learner = M.PPOLearner(pol, learning_rate=3e-4, max_grad_norm=0.5)
    learner.grad_norm.fill_(float("nan"))
    for _ in range(3):
        learner.adam_step()
    torch.cuda.synchronize()
    assert torch.equal(learner.weights.cpu().view(torch.int32), flat.view(torch.int32))
    assert float(learner.grad_norm) == 0.0 and not bool(learner.m.any()) and not bool(learner.v.any())


def _adam_abi_reference(W, seed):
    """three steps on one gradient -> w0, grad and, per step, the three (float64, float32) pairs of w, m, v with the
    max-norm each is measured against (the update w - w0 for the weights, as in the other Adam tests)"""
    import torch

    g = torch.Generator().manual_seed(seed)
    w0, grad = torch.randn(W, generator=g), torch.randn(W, generator=g) * 0.3
    st64, st32 = [], []
    ref64, norms64 = R.adam_reference(w0, [grad] * 3, 1e-3, 1e-5, 0.5, torch.float64, states=st64)
    ref32, _ = R.adam_reference(w0, [grad] * 3, 1e-3, 1e-5, 0.5, torch.float32, states=st32)
    steps = []
    for k in range(3):
        trio = {}
        for name, r64, r32 in (("w", ref64[k], ref32[k]), ("m", st64[k][0], st32[k][0]), ("v", st64[k][1], st32[k][1])):
            scale = float((r64 - w0.double()).abs().max()) if name == "w" else float(r64.abs().max())
            trio[name] = (r64, float((r32.double() - r64).abs().max()) / scale, scale)
        steps.append(trio)
    return w0, grad, steps, norms64


@pytest.mark.parametrize("W", [1, 1025])
def test_adam_step_through_the_abi(W):
    """W = 1 and one past the 1 024-thread stride; grad_norm_out = NULL; nothing outside the W elements is written.
    The rule is that of the other Adam tests: error relative to the max-norm within 4 x torch's float32 error.  With
    W = 1 that yardstick is the rounding of ONE float32, which can be exact by accident, so (as for B <= 2 in the
    gradient tests) it is the largest float32 error over 64 single-weight draws at the same step - torch alone."""
    import ctypes as C

    import torch

    import marl_sortingenv_amd as M

    L = M.load_library()
    w0, grad, steps, norms64 = _adam_abi_reference(W, W)
    e32 = [{name: trio[name][1] for name in trio} for trio in steps]
    if W == 1:
        for seed in range(100, 164):
            other = _adam_abi_reference(W, seed)[2]
            e32 = [{name: max(e[name], o[name][1]) for name in e} for e, o in zip(e32, other)]
    band, sentinel = 32, 12345.0
    bufs = {k: torch.full((W + 2 * band,), sentinel, device="cuda") for k in ("w", "m", "v")}
    bufs["w"][band:band + W] = w0.cuda()
    bufs["m"][band:band + W] = 0.0
    bufs["v"][band:band + W] = 0.0
    grad_dev = grad.cuda()
    norm = torch.full((3,), sentinel, device="cuda")
    ptr = lambda t, off=0: C.c_void_p(t.data_ptr() + 4 * off)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for k in range(3):
        norm_out = None if k == 1 else ptr(norm, 1)
        assert L.mse_ppo_adam_step(W, ptr(bufs["w"], band), ptr(grad_dev), ptr(bufs["m"], band), ptr(bufs["v"], band), k + 1,
                                   1e-3, 0.9, 0.999, 1e-5, 0.5, norm_out, stream) == 0
        torch.cuda.synchronize()
        if k == 1:
            assert float(norm[1]) == sentinel  # NULL: nothing is written
        else:
            assert abs(float(norm[1]) - norms64[k]) <= 4 * np.finfo(np.float32).eps * norms64[k]
            norm[1] = sentinel
        assert norm[0] == sentinel and norm[2] == sentinel
        for name, (r64, _, scale) in steps[k].items():
            err = float((bufs[name][band:band + W].cpu().double() - r64).abs().max()) / scale
            print(f"adam ABI W={W} step {k + 1} {name}: err {err:.3e}, f32 yardstick {e32[k][name]:.3e}")
            assert err <= 4 * e32[k][name], (name, k, err, e32[k][name])
            assert bool((bufs[name][:band] == sentinel).all()) and bool((bufs[name][band + W:] == sentinel).all())


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_load_weights_equals_a_fresh_policy(precision):
    import torch

    import marl_sortingenv_amd as M
    from marl_sortingenv_amd.policy import SB3_KEYS

    D, A = DIMS["mono"]
    pol, flat = _policy("mono", 19, precision=precision)
    new = R.random_flat(D, A, 23)
    pol.load_weights(new)
    fresh = M.MlpPolicy(D, A, dict(zip(SB3_KEYS, R.split(new, D, A))), device=0, precision=precision)
    obs = (torch.rand((5000, D), generator=torch.Generator().manual_seed(1)) * 2 - 1).cuda()
    mask = (torch.rand((5000, A), generator=torch.Generator().manual_seed(2)) < 0.6).cuda()
    mask[:, 0] = True
    a = pol.forward(obs, mask, seed=3, t=4, want_logits=True)
    b = fresh.forward(obs, mask, seed=3, t=4, want_logits=True)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    sd = pol.state_dict()
    assert all(torch.equal(sd[k], w) for k, w in zip(SB3_KEYS, R.split(new, D, A)))
    # by mapping as well
    pol.load_weights(dict(zip(SB3_KEYS, R.split(flat, D, A))))
    assert np.array_equal(pol.flat_weights(), flat.numpy())


def test_load_weights_rechecks_the_f16_range():
    import marl_sortingenv_amd as M
    from marl_sortingenv_amd.policy import SB3_KEYS

    D, A = DIMS["mono"]
    pol, flat = _policy("mono", 29)
    assert pol.precision == "f16x3"
    parts = dict(zip(SB3_KEYS, [p.clone() for p in R.split(flat, D, A)]))
    parts["mlp_extractor.policy_net.2.weight"] *= 3.0e4
    pol.load_weights(parts)
    assert pol.precision == "f32"
    pol.load_weights(flat)
    assert pol.precision == "f16x3"
    pinned, _ = _policy("mono", 29, precision="f16x3")
    with pytest.raises(M.MseError):
        pinned.load_weights(parts)


UPDATE_CFG = dict(kind="mono", n=256, K=16, seed=21, n_epochs=3, batch_size=1024, learning_rate=1e-3)


def _float64_update(flat, data_cpu, perms, cfg, dtype=None, normalize=True):
    """The whole update restated: per minibatch float64 loss + autograd, clip_grad_norm_, Adam(eps=1e-5).  dtype:
    torch.float32 gives the float32 CPU restatement whose drift from the float64 one is the yardstick of the device's."""
    import torch

    D, A = DIMS[cfg["kind"]]
    w = torch.nn.Parameter(flat.to(dtype or torch.float64).clone())
    opt = torch.optim.Adam([w], lr=cfg["learning_rate"], eps=1e-5)
    losses = []
    total = perms[0].numel()
    bs = cfg["batch_size"] if cfg["batch_size"] is not None else (total + 3) // 4  # PPOLearner's documented default
    for perm in perms:
        for start in range(0, perm.numel(), bs):
            rows = perm[start:start + bs]
            args = [t[rows] for t in data_cpu]
            opt.zero_grad()
            loss, _ = R.ppo_loss(w, D, A, *args, HP["clip_range"], HP["ent_coef"], HP["vf_coef"], normalize)
            loss.backward()
            torch.nn.utils.clip_grad_norm_([w], 0.5)
            opt.step()
            losses.append(float(loss.detach()))
    return w.detach(), losses


def test_update_end_to_end():
    import torch

    import marl_sortingenv_amd as M

    cfg = UPDATE_CFG
    D, A = DIMS[cfg["kind"]]
    pol, flat = _policy(cfg["kind"], 31, precision="f32")
    env, col = _rollout(cfg["kind"], cfg["n"], cfg["K"], cfg["seed"], pol)
    learner = M.PPOLearner(pol, learning_rate=cfg["learning_rate"], n_epochs=cfg["n_epochs"], batch_size=cfg["batch_size"],
                           seed=5, **HP)
    data = col.collect()
    out = learner.update(data)
    torch.cuda.synchronize()
    dev_losses = out["stats"][:, 0].cpu().double().numpy()
    data_cpu = _cpu(data)
    all_rows = torch.arange(cfg["n"] * cfg["K"])
    # condition, on the float64 restatement ALONE: the loss on the update's own rollout falls
    w_after64, losses64 = _float64_update(flat, data_cpu, learner.last_permutations, cfg)
    with torch.no_grad():
        before64 = float(R.ppo_loss(flat.double(), D, A, *data_cpu, HP["clip_range"], HP["ent_coef"], HP["vf_coef"])[0])
        after64 = float(R.ppo_loss(w_after64, D, A, *data_cpu, HP["clip_range"], HP["ent_coef"], HP["vf_coef"])[0])
    assert after64 < before64, (before64, after64)
    # the same sign on the device: the kernel's loss over the whole rollout with the weights before / after
    s0, s1 = torch.zeros(8, device="cuda"), torch.zeros(8, device="cuda")
    learner.loss_grad(data, None, all_rows.numel(), s0, weights=flat.cuda(), grad_out=torch.zeros_like(learner.grad))
    learner.loss_grad(data, None, all_rows.numel(), s1, grad_out=torch.zeros_like(learner.grad))
    assert float(s1[0]) < float(s0[0])
    # first minibatch: bound of the loss_grad test; the sequence follows the float64 one (it drifts as f32 steps accumulate)
    rows0 = learner.last_permutations[0][:cfg["batch_size"]]
    args0 = (D, A, *[t[rows0] for t in data_cpu], HP["clip_range"], HP["ent_coef"], HP["vf_coef"])
    _, s64 = R.loss_and_grad(flat, torch.float64, *args0)
    _, s32 = R.loss_and_grad(flat, torch.float32, *args0)
    assert abs(dev_losses[0] - losses64[0]) <= R.stats_bound(s64, s32)[0]
    assert len(dev_losses) == len(losses64) and np.max(np.abs(dev_losses - np.array(losses64))) < 1e-3
    # the policy the rollout kernels read is the updated one
    assert np.array_equal(pol.flat_weights(), learner.weights.cpu().numpy())
    assert float((learner.weights.cpu().double() - w_after64).abs().max()) < 1e-4
    nxt = col.collect()
    K, n = cfg["K"], cfg["n"]
    for k in (0, K - 1):
        again = pol.forward(nxt["observations"][k], nxt["action_masks"][k], seed=col.seed, t=K + k, index_offset=env.index_offset)
        assert torch.equal(again["action"], nxt["actions"][k])
        assert torch.equal(again["logp"], nxt["log_probs"][k]) and torch.equal(again["value"], nxt["values"][k])


# (a) a short last minibatch (4096 = 4 x 1000 + 96), (b) the default batch size, (c) one larger than the rollout, (d) raw
# advantages, (e) the other two env shapes, (f) a policy in the "auto" (f16x3) form
UPDATE_VARIANTS = {
    "short tail": dict(batch_size=1000), "default batch": dict(batch_size=None), "batch > rows": dict(batch_size=5000),
    "raw advantages": dict(normalize=False), "sort": dict(kind="sort"), "press": dict(kind="press"),
    "auto precision": dict(precision="auto"),
}


@pytest.mark.parametrize("variant", list(UPDATE_VARIANTS))
def test_update_configurations(variant):
    """update() against _float64_update in configurations whose drift nobody has measured: the device's distance from
    the float64 update is bounded by 4 x (the rule's factor) the distance of the float32 CPU restatement of the same
    update from it, for the loss sequence and for the weights; both are printed."""
    import torch

    import marl_sortingenv_amd as M
    from marl_sortingenv_amd.policy import SB3_KEYS

    cfg = dict(UPDATE_CFG, normalize=True, precision="f32")
    cfg.update(UPDATE_VARIANTS[variant])
    D, A = DIMS[cfg["kind"]]
    pol, flat = _policy(cfg["kind"], 31, precision=cfg["precision"])
    env, col = _rollout(cfg["kind"], cfg["n"], cfg["K"], cfg["seed"], pol)
    learner = M.PPOLearner(pol, learning_rate=cfg["learning_rate"], n_epochs=cfg["n_epochs"], batch_size=cfg["batch_size"],
                           normalize_advantage=cfg["normalize"], seed=5, **HP)
    data = col.collect()
    out = learner.update(data)
    torch.cuda.synchronize()
    total = cfg["n"] * cfg["K"]
    bs = min(total, cfg["batch_size"] if cfg["batch_size"] is not None else (total + 3) // 4)
    per_epoch = -(-total // bs)
    assert out["stats"].shape == (cfg["n_epochs"] * per_epoch, 8) and learner.step == cfg["n_epochs"] * per_epoch
    assert len(learner.last_permutations) == cfg["n_epochs"]
    assert all(sorted(p.tolist()) == list(range(total)) for p in learner.last_permutations)
    if variant == "default batch":
        assert per_epoch == 4
    if variant == "batch > rows":
        assert per_epoch == 1
    if variant == "short tail":
        assert per_epoch == 5 and total - 4 * bs == 96
    assert set(out["mean"]) == set(R.STAT_NAMES) and R.STAT_NAMES == M.learner.STAT_NAMES
    if not cfg["normalize"]:
        assert out["stats"][:, 6:].cpu().tolist() == [[0.0, 1.0]] * (cfg["n_epochs"] * per_epoch)
    dev_losses = out["stats"][:, 0].cpu().double().numpy()
    data_cpu = _cpu(data)
    w64, l64 = _float64_update(flat, data_cpu, learner.last_permutations, cfg, torch.float64, cfg["normalize"])
    w32, l32 = _float64_update(flat, data_cpu, learner.last_permutations, cfg, torch.float32, cfg["normalize"])
    assert len(dev_losses) == len(l64)
    loss_dev, loss_f32 = np.max(np.abs(dev_losses - np.array(l64))), np.max(np.abs(np.array(l32) - np.array(l64)))
    w_dev, w_f32 = float((learner.weights.cpu().double() - w64).abs().max()), float((w32.double() - w64).abs().max())
    print(f"update [{variant}]: loss sequence device {loss_dev:.3e} / float32 CPU {loss_f32:.3e}; "
          f"weights device {w_dev:.3e} / float32 CPU {w_f32:.3e} (from the float64 update, {len(l64)} minibatches)")
    assert loss_dev <= 4 * loss_f32 and w_dev <= 4 * w_f32
    # the policy the rollout kernels read is the updated one, in whatever form it runs
    assert np.array_equal(pol.flat_weights(), learner.weights.cpu().numpy())
    if cfg["precision"] == "auto":
        assert pol.precision == "f16x3"
    fresh = M.MlpPolicy(D, A, dict(zip(SB3_KEYS, R.split(learner.weights.cpu(), D, A))), device=0, precision=cfg["precision"])
    nxt = col.collect()
    for k in (0, cfg["K"] - 1):
        a = pol.forward(nxt["observations"][k], nxt["action_masks"][k], seed=3, t=k, want_logits=True)
        b = fresh.forward(nxt["observations"][k], nxt["action_masks"][k], seed=3, t=k, want_logits=True)
        for name in a:
            assert torch.equal(a[name], b[name]), (k, name)


def test_learn_is_collect_and_update_alternating():
    import torch

    import marl_sortingenv_amd as M

    cfg = dict(UPDATE_CFG, n_epochs=2)

    def build():
        pol, _ = _policy(cfg["kind"], 31)
        env, col = _rollout(cfg["kind"], cfg["n"], cfg["K"], cfg["seed"], pol)
        return pol, col, M.PPOLearner(pol, learning_rate=cfg["learning_rate"], n_epochs=cfg["n_epochs"],
                                      batch_size=cfg["batch_size"], seed=5, **HP)

    pol_a, col_a, learner_a = build()
    calls = []
    history = learner_a.learn(col_a, 2, callback=lambda it, rec: calls.append((it, dict(rec))))
    pol_b, col_b, learner_b = build()
    stats, rewards = [], []
    for _ in range(2):
        data = col_b.collect()
        stats.append(learner_b.update(data))
        rewards.append(float(data["rewards"].mean()))
    torch.cuda.synchronize()
    for name in ("weights", "m", "v"):
        assert torch.equal(getattr(learner_a, name).view(torch.int32), getattr(learner_b, name).view(torch.int32)), name
    assert learner_a.step == learner_b.step == 2 * cfg["n_epochs"] * 4
    assert np.array_equal(pol_a.flat_weights(), pol_b.flat_weights())
    assert not np.array_equal(pol_a.flat_weights(), _policy(cfg["kind"], 31)[1].numpy())
    assert len(history) == 2 and [c[0] for c in calls] == [0, 1] and [c[1] for c in calls] == history
    for rec, out, reward in zip(history, stats, rewards):
        assert list(rec) == list(M.learner.STAT_NAMES) + ["reward"]
        assert rec["reward"] == reward
        assert [rec[k] for k in M.learner.STAT_NAMES] == out["stats"].mean(dim=0).cpu().tolist()  # bit for bit
        assert all(np.isfinite(v) for v in rec.values())
