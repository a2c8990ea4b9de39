"""Shared by the GPU suites of the PPO learner (not a test module): one mse_ppo_loss_grad call held against the float64
autograd of tests/ppo_reference.py under that file's tolerance rule, and the plumbing around it."""
import numpy as np

from tests import ppo_reference as R

HP = dict(clip_range=0.2, ent_coef=0.05, vf_coef=0.5)
DIMS = {"sort": (13, 2), "press": (16, 11), "mono": (29, 22)}
# (obs_dim, n_actions): every instantiation of k_ppo_grad and every edge of its selector from both sides (the first three
# are the envs' shapes); tests/test_ppo_math_cpu.py asserts that through the selector itself
DIM_MATRIX = [(13, 2), (16, 11), (29, 22), (1, 1), (1, 32), (5, 32), (16, 4), (16, 5), (16, 12), (16, 13), (17, 4),
              (32, 24), (32, 25), (32, 32)]
# pairs one step apart in D or A that the selector must send to two different instantiations
SELECTOR_EDGES = [((16, 4), (16, 5)), ((16, 12), (16, 13)), ((16, 4), (17, 4)), ((32, 24), (32, 25))]


def make_policy(D, A, seed, saturating=False, precision="auto"):
    import marl_sortingenv_amd as M
    from marl_sortingenv_amd.policy import SB3_KEYS

    flat = R.random_flat(D, A, seed, saturating=saturating)
    w = dict(zip(SB3_KEYS, R.split(flat, D, A)))
    return M.MlpPolicy(D, A, w, device=0, precision=precision), flat


def cpu_rows(data, rows=None):
    """flattened CPU copies of the rollout rows (optionally a subset): obs, mask (None without `action_masks`), actions,
    old log-probabilities, advantages, returns"""
    obs = data["observations"].reshape(-1, data["observations"].shape[-1]).cpu()
    mask = data.get("action_masks")
    if mask is not None:
        mask = mask.reshape(-1, mask.shape[-1]).cpu().bool()
    out = [obs, mask] + [data[k].reshape(-1).cpu() for k in ("actions", "log_probs", "advantages", "returns")]
    return [t if rows is None or t is None else t[rows] for t in out]


def device_rows(obs, mk, actions, old_logp, adv, ret):
    """make_rows' CPU tensors -> the dict PPOLearner.loss_grad reads; every buffer exactly n_rows long"""
    import torch

    d = {"observations": obs.contiguous().cuda(), "actions": actions.int().contiguous().cuda(),
         "log_probs": old_logp.contiguous().cuda(), "advantages": adv.contiguous().cuda(), "returns": ret.contiguous().cuda()}
    if mk is not None:
        d["action_masks"] = mk.to(dtype=torch.uint8).contiguous().cuda()
    return d


def random_gae_inputs(K, n, seed, starts="random"):
    """device inputs of mse_gae; starts: "random" (30 % episode starts), "ones" or "zeros" """
    import torch

    g = torch.Generator().manual_seed(seed)
    es = (torch.rand((K, n), generator=g) < 0.3).to(torch.uint8)
    if starts != "random":
        es = torch.full((K, n), 1 if starts == "ones" else 0, dtype=torch.uint8)
    d = {"rewards": torch.randn((K, n), generator=g), "values": torch.randn((K, n), generator=g), "episode_starts": es,
         "last_values": torch.randn((n,), generator=g), "last_dones": (torch.rand((n,), generator=g) < 0.5).to(torch.uint8)}
    return {k: v.cuda() for k, v in d.items()}


def check_loss_grad(D, A, flat, learner, data, rows_cpu, label, yardstick_rows=None, hp=HP, normalize=True, batch=None,
                    ref_args=None, grad_out=None, stats_out=None):
    """one mse_ppo_loss_grad on `rows_cpu` (None: rows 0 .. batch - 1, rows_dev = NULL) against float64 autograd.
    yardstick_rows (B <= 2 only): with one or two rows the float32 yardstick's error is ONE draw of a heavy-tailed
    quantity (saturated units make 1 - h^2 ill-conditioned: the same row gave torch's float32 1.7e-7 and the kernel
    1.3e-6), so the bound takes the largest float32 error among the evaluations of these row sets (each of the batch's
    size) - still torch alone.
    ref_args: the six CPU tensors the reference is evaluated on when they are not simply data[rows_cpu] (clamped
    indices); learner.params must already hold hp / normalize.  grad_out / stats_out: where the first call writes.
    -> (float64 loss, device gradient, device statistics)"""
    import torch

    assert bool(learner.params.normalize_advantage) == bool(normalize)
    total = data["observations"].reshape(-1, D).shape[0]
    stats = torch.zeros(8, device="cuda") if stats_out is None else stats_out
    rows_dev = None if rows_cpu is None else rows_cpu.cuda()
    if batch is None:
        batch = total if rows_cpu is None else rows_cpu.numel()
    w_dev = flat.cuda()
    g = learner.loss_grad(data, rows_dev, batch, stats, weights=w_dev, grad_out=grad_out).clone()
    stats = stats.clone()
    stats2 = torch.zeros(8, device="cuda")
    g2 = learner.loss_grad(data, rows_dev, batch, stats2, weights=w_dev, grad_out=torch.zeros_like(g))
    torch.cuda.synchronize()
    assert torch.equal(g.view(torch.int32), g2.view(torch.int32)) and torch.equal(stats.view(torch.int32), stats2.view(torch.int32)), \
        "two calls with the same inputs must agree bit for bit"
    if ref_args is None:
        ref_args = cpu_rows(data, rows_cpu if rows_cpu is not None else (None if batch == total else torch.arange(batch)))
    tail = (hp["clip_range"], hp["ent_coef"], hp["vf_coef"], normalize)
    args = (D, A, *ref_args, *tail)
    g64, s64 = R.loss_and_grad(flat, torch.float64, *args)
    g32, s32 = R.loss_and_grad(flat, torch.float32, *args)
    scale, allowed = R.grad_bound(g64, g32)
    e32_others = 0.0
    if yardstick_rows is not None:
        for r in yardstick_rows:
            a1 = (D, A, *cpu_rows(data, r.reshape(-1)), *tail)
            (o64, t64), (o32, t32) = R.loss_and_grad(flat, torch.float64, *a1), R.loss_and_grad(flat, torch.float32, *a1)
            allowed = max(allowed, R.grad_bound(o64, o32)[1])
            e32_others = max(e32_others, float((t32.double() - t64).abs().max()))
    err = float((g.cpu().double() - g64).abs().max()) / scale
    serr = np.abs(stats.cpu().double().numpy() - s64.numpy())
    print(f"{label}: kernel grad err {err:.3e}, f32 yardstick {allowed / 4:.3e} (allowed {allowed:.3e}); "
          f"stats err {serr.max():.3e}, f32 stats err {float((s32.double() - s64).abs().max()):.3e}; loss {float(s64[0]):.6f}")
    assert torch.isfinite(g).all() and torch.isfinite(stats).all(), label
    assert err <= allowed, (label, err, allowed)
    assert np.all(serr <= R.stats_bound(s64, s32, e32_others)), (label, stats.cpu(), s64)
    return float(s64[0]), g, stats
