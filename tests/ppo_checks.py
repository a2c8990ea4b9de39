"""Shared by the GPU suites of the PPO learner (not a test module): one mse_ppo_loss_grad call held against the float64
autograd of tests/ppo_reference.py under that file's tolerance rule, and the plumbing around it."""
import numpy as np
import pytest

from tests import ppo_reference as R

HP = dict(clip_range=0.2, ent_coef=0.05, vf_coef=0.5)
DIMS = {"sort": (13, 2), "press": (16, 11), "mono": (29, 22)}
# (obs_dim, n_actions): every instantiation of k_ppo_grad and every edge of its selector from both sides (the first three
# are the envs' shapes); tests/test_ppo_math_cpu.py asserts that through the selector itself
DIM_MATRIX = [(13, 2), (16, 11), (29, 22), (1, 1), (1, 32), (5, 32), (16, 4), (16, 5), (16, 12), (16, 13), (17, 4),
              (32, 24), (32, 25), (32, 32)]
# pairs one step apart in D or A that the selector must send to two different instantiations
SELECTOR_EDGES = [((16, 4), (16, 5)), ((16, 12), (16, 13)), ((16, 4), (17, 4)), ((32, 24), (32, 25))]


ROWS_PER_GROUP = 128  # include/mse.h, mse_ppo_loss_grad: a workgroup of either form takes two tiles of 64 rows per pass


def group_cap():
    """include/mse.h, mse_ppo_loss_grad: min(ceil(batch / 128), 2 * CUs, 512) workgroups of the gradient launch"""
    import torch

    return min(2 * torch.cuda.get_device_properties(0).multi_processor_count, 512)


def bits(t):
    import torch

    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    import torch

    return torch.equal(bits(a), bits(b))


def make_policy(D, A, seed, saturating=False, precision="auto"):
    import marl_sortingenv_amd as M
    from marl_sortingenv_amd.policy import SB3_KEYS

    flat = R.random_flat(D, A, seed, saturating=saturating)
    w = dict(zip(SB3_KEYS, R.split(flat, D, A)))
    return M.MlpPolicy(D, A, w, device=0, precision=precision), flat


def make_learner(D, A, seed, saturating=False, normalize=True, arithmetic="fma"):
    """-> (PPOLearner with HP on a float32 policy of random weights, those weights flat)"""
    import marl_sortingenv_amd as M

    pol, flat = make_policy(D, A, seed, saturating=saturating, precision="f32")
    learner = M.PPOLearner(pol, normalize_advantage=normalize, arithmetic=arithmetic, **HP)
    assert learner.arithmetic == arithmetic
    return learner, flat


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


# ---- what both forms must satisfy: the cases of tests/test_gpu_ppo_shapes.py ("fma") and tests/test_gpu_ppo_matrix.py
# ("matrix"), each defined once; the modules only name them ---------------------------------------------------------------
MONO = DIMS["mono"]


def _cases(*marks):
    """the parametrize marks of one shared test, innermost first: both modules decorate with the same object, so their case
    lists cannot differ"""
    def decorate(fn):
        for mark in marks:
            fn = mark(fn)
        return fn
    return decorate


_param = pytest.mark.parametrize
CASES_EVERY_SHAPE = _cases(_param("D,A", DIM_MATRIX), _param("masked", [True, False]), _param("normalize", [True, False]),
                           _param("saturating", [False, True]))
# both 32-row halves of a tile, a tail in each, an idle tile slot (odd tile counts), a wave of a network without a tile
CASES_BATCH_EDGES = _cases(_param("D,A", [MONO, (32, 32)]), _param("B", [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193]))
SLAB_CAP_OFFSETS = [-1, 0, 1, 65]  # rows beside ROWS_PER_GROUP * group_cap(): see grid_cap
CASES_ROWS_REPEAT = _cases(_param("D,A", [MONO, (32, 32)]))
CASES_ROWS_OUTSIDE = _cases(_param("D,A", [MONO, (32, 32)]), _param("first", ["in range", "clamped pivot"]))
CASES_ACTIONS_OUTSIDE = _cases(_param("D,A", [MONO, (32, 32), (13, 2)]))
CASES_ILLEGAL_ACTION = _cases(_param("D,A", [MONO, (32, 32), (16, 11)]))
CASES_BANDED = _cases(_param("D,A", [MONO, (32, 32), (1, 1)]))


def every_shape_and_option(arithmetic, D, A, masked, normalize, saturating):
    learner, flat = make_learner(D, A, D * 100 + A, saturating=saturating, normalize=normalize, arithmetic=arithmetic)
    obs, mask, mk, *rest = R.make_rows(D, A, 300, seed=11, flat=flat, masked=masked)  # four full tiles and a 44-row tail
    _, _, stats = check_loss_grad(D, A, flat, learner, device_rows(obs, mk, *rest), None, f"{arithmetic} {D}->{A} masked={masked} "
                                  f"normalize={normalize} sat={saturating} B=300", normalize=normalize)
    if not normalize:
        assert stats[6:].tolist() == [0.0, 1.0]


def batch_edges(arithmetic, D, A, B):
    import torch

    learner, flat = make_learner(D, A, 41, arithmetic=arithmetic)
    n_rows = 193 + 128
    obs, mask, mk, *rest = R.make_rows(D, A, n_rows, seed=B, flat=flat, masked=True)
    data = device_rows(obs, mk, *rest)
    perm = torch.randperm(n_rows, generator=torch.Generator().manual_seed(B))
    for rows, name in ((None, "rows_dev=NULL"), (perm[:B], "permuted rows_dev")):
        yard = None
        if B <= 2:  # the largest float32 error over 64 evaluations on other rows is the yardstick
            others = torch.arange(B, B + 64 * B) if rows is None else perm[B:B + 64 * B]
            yard = others.reshape(64, B)
        check_loss_grad(D, A, flat, learner, data, rows, f"{arithmetic} {D}->{A} B={B} {name}", yardstick_rows=yard, batch=B)


def grid_cap(arithmetic, many_rows, B, where):
    """many_rows: (random_flat(*MONO, 43), make_rows of at least B rows).  With cap = group_cap() workgroups of two tile slots:
    at 128 cap rows every slot has one tile; one row more and the first wave takes a second tile with its accumulators
    carried over, 65 more and both slots of workgroup 0 do."""
    D, A = MONO
    flat, (obs, mask, mk, *rest) = many_rows
    assert 0 < B <= obs.shape[0]
    learner, _ = make_learner(D, A, 43, arithmetic=arithmetic)
    data = device_rows(obs[:B], mk[:B], *[t[:B] for t in rest])
    check_loss_grad(D, A, flat, learner, data, None, f"{arithmetic} mono B={B} ({where}, cap {group_cap()})")


def _index_case(arithmetic, D, A, n_rows, seed):
    learner, flat = make_learner(D, A, 47, arithmetic=arithmetic)
    obs, mask, mk, *rest = R.make_rows(D, A, n_rows, seed=seed, flat=flat, masked=True)
    return learner, flat, [obs, mk, *rest]


def rows_may_repeat(arithmetic, D, A):
    import torch

    n_rows = 100
    learner, flat, cpu = _index_case(arithmetic, D, A, n_rows, 1)
    rows = torch.randint(0, n_rows, (3 * n_rows,), generator=torch.Generator().manual_seed(2))
    rows[:4] = 7
    assert rows.unique().numel() < n_rows  # some rows never occur, others repeat
    check_loss_grad(D, A, flat, learner, device_rows(*cpu), rows, f"{arithmetic} {D}->{A} repeated rows, batch = 3 n_rows")


def rows_outside_are_clamped(arithmetic, D, A, first):
    import torch

    n_rows = 100
    learner, flat, cpu = _index_case(arithmetic, D, A, n_rows, 3)
    rows = torch.randperm(n_rows, generator=torch.Generator().manual_seed(4))[:80]
    rows[[5, 17, 40, 79]] = torch.tensor([-5, n_rows, n_rows + 10 ** 9, -2 ** 62])
    if first == "clamped pivot":  # rows[0] is the pivot of the advantage statistics
        rows[0] = n_rows + 10 ** 9
    clamped = rows.clamp(0, n_rows - 1)
    check_loss_grad(D, A, flat, learner, device_rows(*cpu), rows, f"{arithmetic} {D}->{A} rows outside [0, n_rows), first {first}",
                    ref_args=[t[clamped] for t in cpu])


def actions_outside_are_clamped(arithmetic, D, A):
    import torch

    n_rows = 300
    learner, flat, cpu = _index_case(arithmetic, D, A, n_rows, 5)
    obs, mk, actions, *rest = cpu
    mk = mk.clone()
    bad = actions.clone()
    bad[[3, 70, 150]] = -1
    bad[[4, 71, 299]] = A + 3
    bad[200] = 2 ** 31 - 1
    bad[201] = -2 ** 31
    clamped = bad.clamp(0, A - 1)
    mk[torch.arange(n_rows), clamped.long()] = True  # the action clamped to is legal: the illegal ones have their own test
    check_loss_grad(D, A, flat, learner, device_rows(obs, mk, bad, *rest), None, f"{arithmetic} {D}->{A} actions outside [0, A)",
                    ref_args=[obs, mk, clamped, *rest])


def illegal_action(arithmetic, D, A):
    """The reference is R.forward as it is: the logit is -1e8, so is the log-probability, the ratio is 0 and approx_kl
    is of order 1e8 / B."""
    import torch

    n_rows = 300
    learner, flat, cpu = _index_case(arithmetic, D, A, n_rows, 7)
    obs, mk, actions, *rest = cpu
    mk = mk.clone()
    picked = [int(r) for r in torch.nonzero(actions != 0).squeeze(1)[[2, 9, 30]]]  # action 0 stays legal in every row
    for r in picked:
        mk[r, int(actions[r])] = False
    _, _, stats = check_loss_grad(D, A, flat, learner, device_rows(obs, mk, actions, *rest), None,
                                  f"{arithmetic} {D}->{A} {len(picked)} rows with an illegal action")
    assert float(stats[4]) > 1e5  # approx_kl carries the -1e8
    # ... and its float32 error (of order 1e-2) is the largest of the eight, which check_loss_grad's one bound for all
    # statistics inherits; the others are held to the rule with approx_kl left out of the yardstick
    args = (D, A, obs, mk, actions, *rest, HP["clip_range"], HP["ent_coef"], HP["vf_coef"], True)
    s64, s32 = R.loss_and_grad(flat, torch.float64, *args)[1], R.loss_and_grad(flat, torch.float32, *args)[1]
    keep = [0, 1, 2, 3, 5, 6, 7]
    err = np.abs(stats.cpu().double().numpy() - s64.numpy())[keep]
    print(f"{arithmetic} {D}->{A} statistics without approx_kl: err {err.max():.3e}, "
          f"f32 {float((s32.double() - s64)[keep].abs().max()):.3e}")
    assert np.all(err <= R.stats_bound(s64[keep], s32[keep]))


def writes_nothing_else(arithmetic, D, A):
    import torch

    learner, flat = make_learner(D, A, 53, arithmetic=arithmetic)
    obs, mask, mk, *rest = R.make_rows(D, A, 300, seed=9, flat=flat, masked=True)
    W, band, sentinel = flat.numel(), 64, 12345.0
    gbuf = torch.full((W + 2 * band,), sentinel, device="cuda")
    sbuf = torch.full((8 + 2 * band,), sentinel, device="cuda")
    gbuf[band:band + W] = float("nan")
    sbuf[band:band + 8] = float("nan")
    check_loss_grad(D, A, flat, learner, device_rows(obs, mk, *rest), None, f"{arithmetic} {D}->{A} into banded buffers",
                    grad_out=gbuf[band:band + W], stats_out=sbuf[band:band + 8])
    for buf, n in ((gbuf, W), (sbuf, 8)):
        assert bool((buf[:band] == sentinel).all()) and bool((buf[band + n:] == sentinel).all())
        assert int(torch.isfinite(buf[band:band + n]).sum()) == n
