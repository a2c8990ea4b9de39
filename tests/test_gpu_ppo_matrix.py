"""GPU: the matrix-core form of the PPO gradient (PPOLearner(arithmetic="matrix") -> mse_ppo_loss_grad_matrix ->
k_ppo_grad_matrix).  Section 0 names the cases both forms must satisfy (every shape and option, tile edges, the grid cap,
index semantics, writes nothing else), whose bodies and parametrize lists tests/ppo_checks.py defines once; the rest is particular to this form: against
the fma form, its gate, rollouts, update() and the default.  Synthetic rows except where a rollout is named."""
import ctypes as C

import numpy as np
import pytest

from tests import ppo_checks as P
from tests import ppo_reference as R
from tests.ppo_checks import (DIMS, HP, ROWS_PER_GROUP, bits, check_loss_grad, cpu_rows, device_rows, group_cap, make_learner,
                              make_policy, same_bits)

pytestmark = pytest.mark.gpu

MONO = DIMS["mono"]
FORM = "matrix"


# ---- 0. what both forms must satisfy (tests/ppo_checks.py; tests/test_gpu_ppo_shapes.py runs the same with "fma") ---------
@P.CASES_EVERY_SHAPE
def test_every_shape_and_option(D, A, masked, normalize, saturating):
    P.every_shape_and_option(FORM, D, A, masked, normalize, saturating)


@P.CASES_BATCH_EDGES
def test_tile_edges(D, A, B):
    P.batch_edges(FORM, D, A, B)


@pytest.fixture(scope="module")
def many_rows():
    D, A = MONO
    flat = R.random_flat(D, A, 43)
    return flat, R.make_rows(D, A, ROWS_PER_GROUP * group_cap() + 65, seed=5, flat=flat, masked=True)


@pytest.mark.parametrize("off", P.SLAB_CAP_OFFSETS)
def test_grid_cap(many_rows, off):
    P.grid_cap(FORM, many_rows, ROWS_PER_GROUP * group_cap() + off, f"B0{off:+d}")


@P.CASES_ROWS_REPEAT
def test_rows_may_repeat_and_batch_may_exceed_n_rows(D, A):
    P.rows_may_repeat(FORM, D, A)


@P.CASES_ROWS_OUTSIDE
def test_rows_outside_the_rollout_are_clamped(D, A, first):
    P.rows_outside_are_clamped(FORM, D, A, first)


@P.CASES_ACTIONS_OUTSIDE
def test_actions_outside_the_head_are_clamped(D, A):
    P.actions_outside_are_clamped(FORM, D, A)


@P.CASES_ILLEGAL_ACTION
def test_an_action_whose_mask_bit_is_zero(D, A):
    P.illegal_action(FORM, D, A)


@P.CASES_BANDED
def test_writes_its_outputs_and_nothing_else(D, A):
    P.writes_nothing_else(FORM, D, A)


# ---- 1. against the "fma" form ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sort", "press", "mono"])
def test_against_the_fma_form(kind):
    import torch

    D, A = DIMS[kind]
    matrix, flat = make_learner(D, A, 61, arithmetic="matrix")
    fma, _ = make_learner(D, A, 61, arithmetic="fma")
    obs, mask, mk, *rest = R.make_rows(D, A, 300, seed=21, flat=flat, masked=True)
    data = device_rows(obs, mk, *rest)
    out = {}
    for name, learner in (("matrix", matrix), ("fma", fma)):
        stats = torch.zeros(8, device="cuda")
        g = learner.loss_grad(data, None, 300, stats, weights=flat.cuda(), grad_out=torch.zeros(flat.numel(), device="cuda"))
        out[name] = (g, stats)
    torch.cuda.synchronize()
    # the launches around the gradient are the same two kernels
    assert same_bits(out["matrix"][1][6:8], out["fma"][1][6:8])
    # each form is within `allowed` of float64, so the two are within twice that of each other
    tail = (HP["clip_range"], HP["ent_coef"], HP["vf_coef"], True)
    g64, _ = R.loss_and_grad(flat, torch.float64, D, A, obs, mk, *rest, *tail)
    g32, _ = R.loss_and_grad(flat, torch.float32, D, A, obs, mk, *rest, *tail)
    scale, allowed = R.grad_bound(g64, g32)
    diff = float((out["matrix"][0].cpu().double() - out["fma"][0].cpu().double()).abs().max()) / scale
    print(f"{kind}: |matrix - fma| / max|g64| = {diff:.3e}, allowed {2 * allowed:.3e}")
    assert diff <= 2 * allowed


# ---- 2. the gate ----------------------------------------------------------------------------------------------------------------
def test_gate():
    import torch

    D, A = MONO
    learner, flat = make_learner(D, A, 67, arithmetic="matrix")
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
    assert same_bits(g, g0) and same_bits(s, s0)
    # open, a threshold above it: counted, not stopped
    control = torch.zeros(2, dtype=torch.int32, device="cuda")
    g, s = call(control, 2.0 * kl / 1.5)
    assert control.tolist() == [0, 1]
    assert same_bits(g, g0) and same_bits(s, s0)


# ---- 3. rollouts ---------------------------------------------------------------------------------------------------------------
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


# ---- 4. update() ---------------------------------------------------------------------------------------------------------------
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
        assert same_bits(getattr(a, name), getattr(b, name)), (label, name)
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
    assert same_bits(out["stats"], want_stats)
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
    assert same_bits(out["stats"][:j + 1], want_stats[:j + 1])
    assert torch.count_nonzero(bits(out["stats"][j + 1:])) == 0
    assert gated.epochs_done == EPOCHS
    assert np.array_equal(pol.flat_weights().view(np.uint32), gated.weights.cpu().numpy().view(np.uint32))


# ---- 5. the default -----------------------------------------------------------------------------------------------------------
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
    assert same_bits(g, want) and same_bits(stats, want_stats)
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0.0
