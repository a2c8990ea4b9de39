"""GPU: mse_ppo_loss_grad (PPOLearner(arithmetic="fma")) on synthetic rows (tests/ppo_reference.py's make_rows: no env, no
rollout) at every kernel shape, option, batch edge and grid cap, and the index semantics include/mse.h documents.  The
cases (bodies and parametrize lists alike) are defined once for both forms of the gradient launch, in tests/ppo_checks.py
("what both forms must satisfy"); tests/test_gpu_ppo_matrix.py runs the same with arithmetic="matrix".  Every case asserts what check_loss_grad
asserts: float64 autograd under the tolerance rule of tests/ppo_reference.py (4 x the error of torch's own float32 CPU
evaluation, recomputed each run), finite outputs and bit-equal repeat calls."""
import numpy as np
import pytest

from tests import ppo_checks as P
from tests import ppo_reference as R
from tests.ppo_checks import DIMS, ROWS_PER_GROUP, check_loss_grad, device_rows, group_cap, make_learner, random_gae_inputs

pytestmark = pytest.mark.gpu

MONO = DIMS["mono"]
ADV_PARTIAL_ROWS = 256 * 1024  # k_ppo_adv_partial: at most 256 workgroups of 256 threads taking 4 rows each per pass
FORM = "fma"


# ---- shapes -------------------------------------------------------------------------------------------------------------
@P.CASES_EVERY_SHAPE
def test_every_shape_and_option(D, A, masked, normalize, saturating):
    P.every_shape_and_option(FORM, D, A, masked, normalize, saturating)


# ---- batch edges: tile tails, an idle tile slot (odd tile counts), one wave of a network without a tile ------------------
@P.CASES_BATCH_EDGES
def test_batch_edges(D, A, B):
    P.batch_edges(FORM, D, A, B)


# ---- grid caps ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def many_rows():
    D, A = MONO
    flat = R.random_flat(D, A, 43)
    return flat, R.make_rows(D, A, ADV_PARTIAL_ROWS + 1025, seed=5, flat=flat, masked=True)


# the four offsets at the slab cap are ppo_checks.grid_cap's; at 262 144 rows k_ppo_adv_partial's grid stops growing and a
# thread's stride loop goes past its four rows (the same launch stands in front of either form)
CAP_CASES = {**{"slabs" + (f"{off:+d}" if off else ""): ("slabs", off) for off in P.SLAB_CAP_OFFSETS},
             "adv-1": ("adv", -1), "adv": ("adv", 0), "adv+1": ("adv", 1), "adv+1025": ("adv", 1025)}


@pytest.mark.parametrize("where", list(CAP_CASES))
def test_grid_caps(many_rows, where):
    base, off = CAP_CASES[where]
    P.grid_cap(FORM, many_rows, (ROWS_PER_GROUP * group_cap() if base == "slabs" else ADV_PARTIAL_ROWS) + off, where)


# ---- index semantics ------------------------------------------------------------------------------------------------------
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


# ---- nothing outside the outputs is written --------------------------------------------------------------------------------
@P.CASES_BANDED
def test_loss_grad_writes_its_outputs_and_nothing_else(D, A):
    P.writes_nothing_else(FORM, D, A)


def test_gae_writes_its_outputs_and_nothing_else():
    import torch

    import marl_sortingenv_amd as M

    K, n, band, sentinel = 3, 257, 64, 12345.0
    d = random_gae_inputs(K, n, n)
    bufs = [torch.full((K * n + 2 * band,), sentinel, device="cuda") for _ in range(2)]
    for b in bufs:
        b[band:band + K * n] = float("nan")
    d["advantages"], d["returns"] = (b[band:band + K * n].view(K, n) for b in bufs)
    ptrs = [d["advantages"].data_ptr(), d["returns"].data_ptr()]
    M.compute_gae(d, 0.99, 0.95)
    torch.cuda.synchronize()
    assert [d["advantages"].data_ptr(), d["returns"].data_ptr()] == ptrs
    ea, er = R.gae_numpy(*[d[k].cpu().numpy() for k in ("rewards", "values", "episode_starts", "last_values", "last_dones")], 0.99, 0.95)
    assert np.array_equal(d["advantages"].cpu().numpy().view(np.uint32), ea.view(np.uint32))
    assert np.array_equal(d["returns"].cpu().numpy().view(np.uint32), er.view(np.uint32))
    for b in bufs:
        assert bool((b[:band] == sentinel).all()) and bool((b[band + K * n:] == sentinel).all())


# ---- advantage statistics ---------------------------------------------------------------------------------------------------
def _ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


@pytest.mark.parametrize("case", ["normal", "offset 1000", "constant 0.75", "constant 1000.1", "two rows", "pivot +100"])
def test_advantage_mean_and_std(case):
    """stats_out[6:8] against numpy float64 on the float32 advantages.  The bound is derived: the kernel forms
    d = a - pivot exactly in double (pivot = the first row's advantage), sums d and d^2 along chains of fewer than 512
    additions and rounds once to float32.  So the mean is within 1 ulp of float32, and the std within 1 ulp of float32
    plus  std * 512 * 2^-52 * (1 + (pivot - mean)^2 / var)  for the cancellation in  q - s^2 / B.  A constant vector
    gives exactly 0."""
    import torch

    D, A = MONO
    learner, flat = make_learner(D, A, 59)
    B = 2 if case == "two rows" else 300
    n_rows = B + (128 if B == 2 else 0)
    obs, mask, mk, actions, old_logp, adv, ret = R.make_rows(D, A, n_rows, seed=13, flat=flat, masked=True)
    noise = torch.randn(n_rows, generator=torch.Generator().manual_seed(17))
    if case in ("normal", "two rows"):
        adv = noise
    elif case == "offset 1000":
        adv = 1000.0 + 0.01 * noise
    elif case.startswith("constant"):
        adv = torch.full((n_rows,), float(case.split()[1]))
    else:
        adv = noise.clone()
        adv[0] = 100.0
    adv = adv.float()
    yard = torch.arange(2, 130).reshape(64, 2) if B == 2 else None
    _, g, stats = check_loss_grad(D, A, flat, learner, device_rows(obs, mk, actions, old_logp, adv, ret), None,
                                  f"advantages: {case}", yardstick_rows=yard, batch=B)
    a = adv[:B].numpy().astype(np.float64)
    mean, std, var, pivot = a.mean(), a.std(ddof=1), a.var(ddof=1), a[0]
    got_mean, got_std = float(stats[6]), float(stats[7])
    print(f"advantages: {case}: mean {got_mean!r} (float64 {mean!r}), std {got_std!r} (float64 {std!r})")
    if case.startswith("constant"):
        assert got_std == 0.0 and got_mean == float(adv[0])
        assert bool(torch.isfinite(g).all())
        return
    assert abs(got_mean - mean) <= _ulp32(mean)
    assert abs(got_std - std) <= _ulp32(std) + std * 512 * 2.0 ** -52 * (1.0 + (pivot - mean) ** 2 / var)
