"""GPU: the on-device PPO learner (mse_gae, mse_ppo_loss_grad, mse_ppo_adam_step, mse_policy_set_weights, PPOLearner)
against tests/ppo_reference.py - numpy float32 for GAE (bit-equal), float64 torch autograd for the loss and gradient,
float64 clip_grad_norm_ + Adam.  Tolerances: the rule written in tests/ppo_reference.py (4 x the error of torch's own
float32 CPU evaluation against float64, computed each run; nothing is taken from the kernels)."""
import numpy as np
import pytest

from tests import ppo_reference as R

pytestmark = pytest.mark.gpu

HP = dict(clip_range=0.2, ent_coef=0.05, vf_coef=0.5)
DIMS = {"sort": (13, 2), "press": (16, 11), "mono": (29, 22)}


def _policy(kind, seed, saturating=False, precision="auto"):
    import marl_sortingenv_amd as M
    from marl_sortingenv_amd.policy import SB3_KEYS

    D, A = DIMS[kind]
    flat = R.random_flat(D, A, seed, saturating=saturating)
    w = dict(zip(SB3_KEYS, R.split(flat, D, A)))
    return M.MlpPolicy(D, A, w, device=0, precision=precision), flat


def _rollout(kind, n, K, seed, policy, max_steps=5):
    import marl_sortingenv_amd as M

    env = M.BatchedSortingEnv(kind=kind, num_envs=n, device=0, base_seed=seed, max_steps=max_steps, noise_sorting=0.05,
                              balesize=200, auto_reset=True)
    col = M.FusedPolicyRollout(env, policy, K, seed=seed + 1)
    return env, col


def _cpu(data, rows=None):
    """flattened CPU copies of the rollout rows (optionally a subset)"""
    obs = data["observations"].reshape(-1, data["observations"].shape[-1]).cpu()
    mask = data["action_masks"].reshape(-1, data["action_masks"].shape[-1]).cpu().bool()
    out = [obs, mask] + [data[k].reshape(-1).cpu() for k in ("actions", "log_probs", "advantages", "returns")]
    return [t if rows is None else t[rows] for t in out]


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


@pytest.mark.parametrize("n", [1, 63])
def test_gae_on_random_inputs(n):
    import torch

    import marl_sortingenv_amd as M

    K = 9
    g = torch.Generator().manual_seed(n)
    d = {"rewards": torch.randn((K, n), generator=g), "values": torch.randn((K, n), generator=g),
         "episode_starts": (torch.rand((K, n), generator=g) < 0.3).to(torch.uint8),
         "last_values": torch.randn((n,), generator=g), "last_dones": (torch.rand((n,), generator=g) < 0.5).to(torch.uint8)}
    d = {k: v.cuda() for k, v in d.items()}
    for gamma, lam in ((0.99, 0.95), (0.9, 1.0)):
        M.compute_gae(d, gamma, lam)
        ea, er = R.gae_numpy(*_gae_inputs_numpy(d), gamma, lam)
        assert np.array_equal(d["advantages"].cpu().numpy().view(np.uint32), ea.view(np.uint32))
        assert np.array_equal(d["returns"].cpu().numpy().view(np.uint32), er.view(np.uint32))


def _check_loss_grad(kind, flat, learner, data, rows_cpu, label, yardstick_rows=None):
    """one mse_ppo_loss_grad on `rows_cpu` (None: the whole rollout, rows_dev = NULL) against float64 autograd.
    yardstick_rows (B = 1 only): with a single row the float32 yardstick's error is ONE draw of a heavy-tailed quantity
    (saturated units make 1 - h^2 ill-conditioned: the same row gave torch's float32 1.7e-7 and the kernel 1.3e-6), so
    the bound takes the largest float32 error among the single-row evaluations of these rows - still torch alone."""
    import torch

    D, A = DIMS[kind]
    total = data["rewards"].numel()
    stats = torch.zeros(8, device="cuda")
    rows_dev = None if rows_cpu is None else rows_cpu.cuda()
    batch = total if rows_cpu is None else rows_cpu.numel()
    w_dev = flat.cuda()
    g = learner.loss_grad(data, rows_dev, batch, stats, weights=w_dev).clone()
    stats2 = torch.zeros(8, device="cuda")
    g2 = learner.loss_grad(data, rows_dev, batch, stats2, weights=w_dev, grad_out=torch.zeros_like(g))
    torch.cuda.synchronize()
    assert torch.equal(g.view(torch.int32), g2.view(torch.int32)) and torch.equal(stats.view(torch.int32), stats2.view(torch.int32)), \
        "two calls with the same inputs must agree bit for bit"
    obs, mask, actions, old_logp, adv, ret = _cpu(data, rows_cpu)
    args = (D, A, obs, mask, actions, old_logp, adv, ret, HP["clip_range"], HP["ent_coef"], HP["vf_coef"])
    g64, s64 = R.loss_and_grad(flat, torch.float64, *args)
    g32, s32 = R.loss_and_grad(flat, torch.float32, *args)
    scale, allowed = R.grad_bound(g64, g32)
    if yardstick_rows is not None:
        for r in yardstick_rows:
            a1 = (D, A, *_cpu(data, r.reshape(1)), HP["clip_range"], HP["ent_coef"], HP["vf_coef"])
            allowed = max(allowed, R.grad_bound(R.loss_and_grad(flat, torch.float64, *a1)[0],
                                                R.loss_and_grad(flat, torch.float32, *a1)[0])[1])
    err = float((g.cpu().double() - g64).abs().max()) / scale
    serr = np.abs(stats.cpu().double().numpy() - s64.numpy())
    print(f"{label}: kernel grad err {err:.3e}, f32 yardstick {allowed / 4:.3e} (allowed {allowed:.3e}); "
          f"stats err {serr.max():.3e}, f32 stats err {float((s32.double() - s64).abs().max()):.3e}; loss {float(s64[0]):.6f}")
    assert err <= allowed, (label, err, allowed)
    assert np.all(serr <= R.stats_bound(s64, s32)), (label, stats.cpu(), s64)
    return float(s64[0])


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


def test_adam_step_matches_torch_float64():
    import torch

    import marl_sortingenv_amd as M

    pol, flat = _policy("mono", 17)
    W = flat.numel()
    for max_norm, gscale in ((0.5, 5.0), (0.5, 1e-3), (0.0, 1.0)):  # norm above / below max_grad_norm, no clipping
        learner = M.PPOLearner(pol, learning_rate=3e-4, max_grad_norm=max_norm)
        g = torch.Generator().manual_seed(5)
        grads = [torch.randn(W, generator=g) * gscale / W ** 0.5 for _ in range(20)]
        ref64, norms64 = R.adam_reference(flat, grads, 3e-4, 1e-5, max_norm, torch.float64)
        ref32, _ = R.adam_reference(flat, grads, 3e-4, 1e-5, max_norm, torch.float32)
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
            assert abs(float(learner.grad_norm.cpu()) - norms64[k]) <= 4 * np.finfo(np.float32).eps * norms64[k]
        assert (norms64[0] > max_norm) == (gscale == 5.0) or max_norm == 0.0


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


def _float64_update(flat, data_cpu, perms, cfg):
    """The whole update restated: per minibatch float64 loss + autograd, clip_grad_norm_, Adam(eps=1e-5)."""
    import torch

    D, A = DIMS[cfg["kind"]]
    w = torch.nn.Parameter(flat.double().clone())
    opt = torch.optim.Adam([w], lr=cfg["learning_rate"], eps=1e-5)
    losses = []
    bs = cfg["batch_size"]
    for perm in perms:
        for start in range(0, perm.numel(), bs):
            rows = perm[start:start + bs]
            args = [t[rows] for t in data_cpu]
            opt.zero_grad()
            loss, _ = R.ppo_loss(w, D, A, *args, HP["clip_range"], HP["ent_coef"], HP["vf_coef"])
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
