"""GPU: the matrix-core form of the PPO gradient (PPOLearner(arithmetic="matrix") -> mse_ppo_loss_grad_matrix ->
k_ppo_grad_matrix) under the rule every other form is held to: float64 autograd from tests/ppo_reference.py, 4 x the error
of torch's own float32 CPU evaluation recomputed each run, `stats_bound` for the statistics, bit-equal repeat calls
(tests/ppo_checks.py: check_loss_grad).  Synthetic rows except where a rollout is named."""
import ctypes as C

import numpy as np
import pytest

from tests import ppo_reference as R
from tests.ppo_checks import DIM_MATRIX, DIMS, HP, check_loss_grad, cpu_rows, device_rows, make_policy

pytestmark = pytest.mark.gpu

MONO = DIMS["mono"]
ROWS_PER_GROUP = 128  # include/mse.h, mse_ppo_loss_grad_matrix: a workgroup takes two tiles of 64 rows per pass


def _group_cap():
    """include/mse.h, mse_ppo_loss_grad_matrix: min(ceil(batch / 128), 2 * CUs, 512) workgroups"""
    import torch

    return min(2 * torch.cuda.get_device_properties(0).multi_processor_count, 512)


def _learner(D, A, seed, saturating=False, normalize=True, arithmetic="matrix"):
    import marl_sortingenv_amd as M

    pol, flat = make_policy(D, A, seed, saturating=saturating, precision="f32")
    learner = M.PPOLearner(pol, normalize_advantage=normalize, arithmetic=arithmetic, **HP)
    assert learner.arithmetic == arithmetic
    return learner, flat


def _bits(t):
    import torch

    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    import torch

    return torch.equal(_bits(a), _bits(b))


# ---- 1. every shape and option --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("saturating", [False, True])
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("D,A", DIM_MATRIX)
def test_every_shape_and_option(D, A, masked, normalize, saturating):
    learner, flat = _learner(D, A, D * 100 + A, saturating=saturating, normalize=normalize)
    obs, mask, mk, *rest = R.make_rows(D, A, 300, seed=11, flat=flat, masked=masked)  # four full tiles and a 44-row tail
    _, _, stats = check_loss_grad(D, A, flat, learner, device_rows(obs, mk, *rest), None,
                                  f"matrix {D}->{A} masked={masked} normalize={normalize} sat={saturating} B=300", normalize=normalize)
    if not normalize:
        assert stats[6:].tolist() == [0.0, 1.0]


# ---- 2. tile edges: both 32-row halves of a tile, a tail in each, an idle tile slot, a wave with no tile ---------------------
@pytest.mark.parametrize("B", [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 193])
@pytest.mark.parametrize("D,A", [MONO, (32, 32)])
def test_tile_edges(D, A, B):
    import torch

    learner, flat = _learner(D, A, 41)
    n_rows = 321
    obs, mask, mk, *rest = R.make_rows(D, A, n_rows, seed=B, flat=flat, masked=True)
    data = device_rows(obs, mk, *rest)
    perm = torch.randperm(n_rows, generator=torch.Generator().manual_seed(B))
    for rows, name in ((None, "rows_dev=NULL"), (perm[:B], "permuted rows_dev")):
        yard = None
        if B <= 2:  # the largest float32 error over 64 evaluations on other rows is the yardstick
            others = torch.arange(B, B + 64 * B) if rows is None else perm[B:B + 64 * B]
            yard = others.reshape(64, B)
        check_loss_grad(D, A, flat, learner, data, rows, f"matrix {D}->{A} B={B} {name}", yardstick_rows=yard, batch=B)


# ---- 3. the grid cap ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def many_rows():
    D, A = MONO
    flat = R.random_flat(D, A, 43)
    return flat, R.make_rows(D, A, ROWS_PER_GROUP * _group_cap() + 65, seed=5, flat=flat, masked=True)


# B0 rows: every tile slot of the capped grid has one tile; one row more and the first wave takes a second tile with its
# accumulators carried over, 65 more and both slots of workgroup 0 do
@pytest.mark.parametrize("off", [-1, 0, 1, 65])
def test_grid_cap(many_rows, off):
    D, A = MONO
    flat, (obs, mask, mk, *rest) = many_rows
    B = ROWS_PER_GROUP * _group_cap() + off
    assert 0 < B <= obs.shape[0]
    learner, _ = _learner(D, A, 43)
    data = device_rows(obs[:B], mk[:B], *[t[:B] for t in rest])
    check_loss_grad(D, A, flat, learner, data, None, f"matrix mono B={B} (B0{off:+d}, cap {_group_cap()})")


# ---- 4. index semantics -------------------------------------------------------------------------------------------------------
def _index_case(D, A, n_rows, seed):
    learner, flat = _learner(D, A, 47)
    obs, mask, mk, *rest = R.make_rows(D, A, n_rows, seed=seed, flat=flat, masked=True)
    return learner, flat, [obs, mk, *rest]


@pytest.mark.parametrize("D,A", [MONO, (32, 32)])
def test_rows_may_repeat_and_batch_may_exceed_n_rows(D, A):
    import torch

    n_rows = 100
    learner, flat, cpu = _index_case(D, A, n_rows, 1)
    rows = torch.randint(0, n_rows, (3 * n_rows,), generator=torch.Generator().manual_seed(2))
    rows[:4] = 7
    assert rows.unique().numel() < n_rows
    check_loss_grad(D, A, flat, learner, device_rows(*cpu), rows, f"matrix {D}->{A} repeated rows, batch = 3 n_rows")


@pytest.mark.parametrize("first", ["in range", "clamped pivot"])
def test_rows_outside_the_rollout_are_clamped(first):
    import torch

    D, A = MONO
    n_rows = 100
    learner, flat, cpu = _index_case(D, A, n_rows, 3)
    rows = torch.randperm(n_rows, generator=torch.Generator().manual_seed(4))[:80]
    rows[[5, 17, 40, 79]] = torch.tensor([-5, n_rows, n_rows + 10 ** 9, -2 ** 62])
    if first == "clamped pivot":  # rows[0] is the pivot of the advantage statistics
        rows[0] = n_rows + 10 ** 9
    clamped = rows.clamp(0, n_rows - 1)
    check_loss_grad(D, A, flat, learner, device_rows(*cpu), rows, f"matrix rows outside [0, n_rows), first {first}",
                    ref_args=[t[clamped] for t in cpu])


def test_actions_outside_the_head_are_clamped():
    import torch

    D, A = MONO
    n_rows = 300
    learner, flat, cpu = _index_case(D, A, n_rows, 5)
    obs, mk, actions, *rest = cpu
    mk = mk.clone()
    bad = actions.clone()
    bad[[3, 70, 150]] = -1
    bad[[4, 71, 299]] = A + 3
    bad[200] = 2 ** 31 - 1
    bad[201] = -2 ** 31
    clamped = bad.clamp(0, A - 1)
    mk[torch.arange(n_rows), clamped.long()] = True  # the action clamped to is legal: the illegal ones have their own test
    check_loss_grad(D, A, flat, learner, device_rows(obs, mk, bad, *rest), None, "matrix actions outside [0, A)",
                    ref_args=[obs, mk, clamped, *rest])


def test_an_action_whose_mask_bit_is_zero():
    """The reference is R.forward as it is: the logit is -1e8, so is the log-probability, the ratio is 0."""
    import torch

    D, A = MONO
    n_rows = 300
    learner, flat, cpu = _index_case(D, A, n_rows, 7)
    obs, mk, actions, *rest = cpu
    mk = mk.clone()
    picked = [int(r) for r in torch.nonzero(actions != 0).squeeze(1)[[2, 9, 30]]]  # action 0 stays legal in every row
    for r in picked:
        mk[r, int(actions[r])] = False
    _, _, stats = check_loss_grad(D, A, flat, learner, device_rows(obs, mk, actions, *rest), None,
                                  f"matrix {len(picked)} rows with an illegal action")
    assert float(stats[4]) > 1e5  # approx_kl carries the -1e8


# ---- 5. outputs and nothing else -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,A", [MONO, (1, 1)])
def test_writes_its_outputs_and_nothing_else(D, A):
    import torch

    learner, flat = _learner(D, A, 53)
    obs, mask, mk, *rest = R.make_rows(D, A, 300, seed=9, flat=flat, masked=True)
    W, band, sentinel = flat.numel(), 64, 12345.0
    gbuf = torch.full((W + 2 * band,), sentinel, device="cuda")
    sbuf = torch.full((8 + 2 * band,), sentinel, device="cuda")
    gbuf[band:band + W] = float("nan")
    sbuf[band:band + 8] = float("nan")
    check_loss_grad(D, A, flat, learner, device_rows(obs, mk, *rest), None, f"matrix {D}->{A} into banded buffers",
                    grad_out=gbuf[band:band + W], stats_out=sbuf[band:band + 8])
    for buf, n in ((gbuf, W), (sbuf, 8)):
        assert bool((buf[:band] == sentinel).all()) and bool((buf[band + n:] == sentinel).all())
        assert int(torch.isfinite(buf[band:band + n]).sum()) == n


# ---- 6. against the "fma" form ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sort", "press", "mono"])
def test_against_the_fma_form(kind):
    import torch

    D, A = DIMS[kind]
    matrix, flat = _learner(D, A, 61)
    fma, _ = _learner(D, A, 61, arithmetic="fma")
    obs, mask, mk, *rest = R.make_rows(D, A, 300, seed=21, flat=flat, masked=True)
    data = device_rows(obs, mk, *rest)
    out = {}
    for name, learner in (("matrix", matrix), ("fma", fma)):
        stats = torch.zeros(8, device="cuda")
        g = learner.loss_grad(data, None, 300, stats, weights=flat.cuda(), grad_out=torch.zeros(flat.numel(), device="cuda"))
        out[name] = (g, stats)
    torch.cuda.synchronize()
    # the launches around the gradient are the same two kernels
    assert _same_bits(out["matrix"][1][6:8], out["fma"][1][6:8])
    # each form is within `allowed` of float64, so the two are within twice that of each other
    tail = (HP["clip_range"], HP["ent_coef"], HP["vf_coef"], True)
    g64, _ = R.loss_and_grad(flat, torch.float64, D, A, obs, mk, *rest, *tail)
    g32, _ = R.loss_and_grad(flat, torch.float32, D, A, obs, mk, *rest, *tail)
    scale, allowed = R.grad_bound(g64, g32)
    diff = float((out["matrix"][0].cpu().double() - out["fma"][0].cpu().double()).abs().max()) / scale
    print(f"{kind}: |matrix - fma| / max|g64| = {diff:.3e}, allowed {2 * allowed:.3e}")
    assert diff <= 2 * allowed


# ---- 7. the gate ----------------------------------------------------------------------------------------------------------------
def test_gate():
    import torch

    D, A = MONO
    learner, flat = _learner(D, A, 67)
    obs, mask, mk, *rest = R.make_rows(D, A, 300, seed=23, flat=flat, masked=True)
    data = device_rows(obs, mk, *rest)
    w = flat.cuda()
    nan = float("nan")

    def call(control, target_kl):
        g, s = torch.full((flat.numel(),), nan, device="cuda"), torch.full((8,), nan, device="cuda")
        learner.loss_grad(data, None, 300, s, weights=w, grad_out=g, control=control, target_kl=target_kl)
        torch.cuda.synchronize()
        return g, s

    g0, s0 = call(None, 0.0)  # the ungated dry run
    kl = float(s0[4])
    assert kl > 0.0 and bool(torch.isfinite(g0).all())
    # closed on entry: nothing is written, the block is unchanged
    control = torch.tensor([1, 5], dtype=torch.int32, device="cuda")
    g, s = call(control, 1e9)
    assert control.tolist() == [1, 5]
    assert bool(torch.isnan(g).all()) and bool(torch.isnan(s).all())
    # open, a threshold below this minibatch's approx_kl: the minibatch is counted and the flag set
    control = torch.zeros(2, dtype=torch.int32, device="cuda")
    g, s = call(control, 0.5 * kl / 1.5)
    assert control.tolist() == [1, 1]
    assert _same_bits(g, g0) and _same_bits(s, s0)
    # open, a threshold above it: counted, not stopped
    control = torch.zeros(2, dtype=torch.int32, device="cuda")
    g, s = call(control, 2.0 * kl / 1.5)
    assert control.tolist() == [0, 1]
    assert _same_bits(g, g0) and _same_bits(s, s0)


# ---- 8. rollouts ---------------------------------------------------------------------------------------------------------------
def _rollout(kind, pol, n=256, K=4, seed=21):
    import marl_sortingenv_amd as M

    env = M.BatchedSortingEnv(kind=kind, num_envs=n, device=0, base_seed=seed, max_steps=5, noise_sorting=0.05, balesize=200,
                              auto_reset=True)
    return env, M.FusedPolicyRollout(env, pol, K, seed=seed + 1)


@pytest.mark.parametrize("kind", ["sort", "press", "mono"])
def test_on_a_rollout(kind):
    import torch

    import marl_sortingenv_amd as M

    D, A = DIMS[kind]
    pol, flat = make_policy(D, A, 31)
    learner = M.PPOLearner(pol, arithmetic="matrix", **HP)
    _, col = _rollout(kind, pol)
    data = M.compute_gae(col.collect(), learner.gamma, learner.gae_lambda)
    check_loss_grad(D, A, flat, learner, data, None, f"matrix {kind} rollout, all 1024 rows")
    perm = torch.randperm(1024, generator=torch.Generator().manual_seed(3))[:400]
    check_loss_grad(D, A, flat, learner, data, perm, f"matrix {kind} rollout, 400 permuted rows")


# ---- 9. update() ---------------------------------------------------------------------------------------------------------------
N_ENVS, K_STEPS, EPOCHS, BS, SEED = 256, 4, 2, 400, 5
TOTAL = N_ENVS * K_STEPS
M_UPDATE = EPOCHS * -(-TOTAL // BS)  # six minibatches: 400, 400, 224 rows per epoch


def _update_setup(lr=1e-3, **kw):
    import marl_sortingenv_amd as M

    pol, flat = make_policy(*MONO, 31)
    _, col = _rollout("mono", pol)
    learner = M.PPOLearner(pol, learning_rate=lr, n_epochs=EPOCHS, batch_size=BS, seed=SEED, arithmetic="matrix", shuffle="device",
                           **HP, **kw)
    return pol, flat, col, learner


def _update_by_hand(hand, data, target_kl=None):
    """update() from permutation(), loss_grad() and adam_step(), ungated; with target_kl one host read per minibatch and
    SB3's rule.  -> (stats with NaN in the rows that did not run, minibatches run, stopped)"""
    import torch

    import marl_sortingenv_amd as M

    M.compute_gae(data, hand.gamma, hand.gae_lambda)
    stats = torch.full((M_UPDATE, 8), float("nan"), device="cuda")
    perms = [hand.permutation(TOTAL, hand.epochs_done + e) for e in range(EPOCHS)]
    hand.epochs_done += EPOCHS
    i = 0
    for perm in perms:
        rows = perm.cuda()
        for start in range(0, TOTAL, BS):
            mb = rows[start:start + BS]
            hand.loss_grad(data, mb, mb.numel(), stats[i])
            i += 1
            if target_kl is not None and float(stats[i - 1, 4].item()) > 1.5 * target_kl:
                return stats, i, True
            hand.adam_step()
    return stats, i, False


def _assert_same_learner(a, b, label):
    for name in ("weights", "m", "v"):
        assert _same_bits(getattr(a, name), getattr(b, name)), (label, name)
    assert a.step == b.step, label


@pytest.fixture(scope="module")
def update_rollout():
    _, _, col, _ = _update_setup()
    return {k: v.clone() for k, v in col.collect().items()}


def test_update_equals_the_hand_loop_and_follows_float64(update_rollout):
    import torch

    from tests.test_gpu_ppo import _float64_update

    data = {k: v.clone() for k, v in update_rollout.items()}
    pol, flat, _, learner = _update_setup()
    _, _, _, hand = _update_setup()
    out = learner.update(data)
    want_stats, run, stopped = _update_by_hand(hand, data)
    torch.cuda.synchronize()
    assert (run, stopped) == (M_UPDATE, False) and learner.step == M_UPDATE
    _assert_same_learner(learner, hand, "update")
    assert _same_bits(out["stats"], want_stats)
    assert np.array_equal(pol.flat_weights(), learner.weights.cpu().numpy())
    # the float64 update on the same permutations, by test_update_end_to_end's rule
    cfg = dict(kind="mono", batch_size=BS, learning_rate=1e-3)
    perms = [learner.permutation(TOTAL, e) for e in learner.last_epochs]
    w64, losses64 = _float64_update(flat, cpu_rows(data), perms, cfg)
    dev_losses = out["stats"][:, 0].cpu().double().numpy()
    assert len(dev_losses) == len(losses64) and np.max(np.abs(dev_losses - np.array(losses64))) < 1e-3
    assert float((learner.weights.cpu().double() - w64).abs().max()) < 1e-4


def test_update_with_target_kl_stops_where_the_hand_loop_stops(update_rollout):
    import torch

    LR_RISING = 3e-4  # small enough that approx_kl keeps rising over the Adam steps of an update
    data = {k: v.clone() for k, v in update_rollout.items()}
    _, _, _, dry = _update_setup(lr=LR_RISING)
    kl = dry.update(data)["stats"][:, 4].cpu().tolist()
    print("approx_kl of the ungated update:", kl)
    rising = [j for j in range(M_UPDATE // 2, M_UPDATE - 1) if kl[j] > max(kl[:j])]  # inside the second epoch
    assert rising, "approx_kl never rises above its past inside the second epoch: no stop to test"
    j = rising[-1]
    target_kl = 0.5 * (max(kl[:j]) + kl[j]) / 1.5
    assert max(kl[:j]) < 1.5 * target_kl < kl[j]
    pol, _, _, gated = _update_setup(lr=LR_RISING, target_kl=target_kl)
    _, _, _, hand = _update_setup(lr=LR_RISING)
    out = gated.update(data)
    want_stats, want_run, want_stopped = _update_by_hand(hand, data, target_kl)
    torch.cuda.synchronize()
    assert want_stopped and want_run == j + 1
    assert out["stopped"] is True and out["minibatches_run"] == j + 1
    _assert_same_learner(gated, hand, "gated update")
    assert gated.step == j  # Adam steps taken: the stopping minibatch took none
    assert _same_bits(out["stats"][:j + 1], want_stats[:j + 1])
    assert torch.count_nonzero(_bits(out["stats"][j + 1:])) == 0
    assert gated.epochs_done == EPOCHS
    assert np.array_equal(pol.flat_weights().view(np.uint32), gated.weights.cpu().numpy().view(np.uint32))


# ---- 10. the default -----------------------------------------------------------------------------------------------------------
def test_the_default_is_the_fma_form():
    import torch

    import marl_sortingenv_amd as M

    D, A = MONO
    pol, flat = make_policy(D, A, 71, precision="f32")
    learner = M.PPOLearner(pol)
    assert learner.arithmetic == "fma"
    obs, mask, mk, *rest = R.make_rows(D, A, 300, seed=25, flat=flat, masked=True)
    data = device_rows(obs, mk, *rest)
    stats, want_stats = torch.zeros(8, device="cuda"), torch.zeros(8, device="cuda")
    g = learner.loss_grad(data, None, 300, stats)
    want = torch.zeros_like(g)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    status = learner.L.mse_ppo_loss_grad(D, A, ptr(learner.weights), 300, None, 300, ptr(data["observations"]), ptr(data["action_masks"]),
                                         ptr(data["actions"]), ptr(data["log_probs"]), ptr(data["advantages"]), ptr(data["returns"]),
                                         C.byref(learner.params), ptr(want), ptr(want_stats), ptr(learner.workspace),
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert status == 0
    assert _same_bits(g, want) and _same_bits(stats, want_stats)
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0.0
