"""GPU: mse_ppo_loss_grad on synthetic rows (tests/ppo_reference.py's make_rows: no env, no rollout) at every kernel
shape, option, batch edge and grid cap, and the index semantics include/mse.h documents.  Every case asserts what
tests/ppo_checks.py's check_loss_grad asserts: float64 autograd under the tolerance rule of tests/ppo_reference.py
(4 x the error of torch's own float32 CPU evaluation, recomputed each run) and bit-equal repeat calls."""
import numpy as np
import pytest

from tests import ppo_reference as R
from tests.ppo_checks import DIM_MATRIX, DIMS, HP, check_loss_grad, device_rows, make_policy, random_gae_inputs

pytestmark = pytest.mark.gpu

MONO = DIMS["mono"]
ADV_PARTIAL_ROWS = 256 * 1024  # k_ppo_adv_partial: at most 256 workgroups of 256 threads taking 4 rows each per pass


def _learner(D, A, seed, saturating=False, normalize=True):
    import marl_sortingenv_amd as M

    pol, flat = make_policy(D, A, seed, saturating=saturating, precision="f32")
    return M.PPOLearner(pol, normalize_advantage=normalize, **HP), flat


def _slab_cap():
    import torch

    return min(2 * torch.cuda.get_device_properties(0).multi_processor_count, 512)  # workgroups of k_ppo_grad at most


# ---- shapes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("saturating", [False, True])
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("D,A", DIM_MATRIX)
def test_every_shape_and_option(D, A, masked, normalize, saturating):
    learner, flat = _learner(D, A, D * 100 + A, saturating=saturating, normalize=normalize)
    obs, mask, mk, *rest = R.make_rows(D, A, 300, seed=11, flat=flat, masked=masked)
    data = device_rows(obs, mk, *rest)
    _, _, stats = check_loss_grad(D, A, flat, learner, data, None, f"{D}->{A} masked={masked} normalize={normalize} "
                                  f"sat={saturating} B=300", normalize=normalize)
    if not normalize:
        assert stats[6:].tolist() == [0.0, 1.0]


# ---- batch edges: tile tails, an idle tile slot (odd tile counts), one wave of a network without a tile ------------------
@pytest.mark.parametrize("B", [2, 63, 64, 65, 127, 128, 129, 191, 192, 193])
@pytest.mark.parametrize("D,A", [MONO, (32, 32)])
def test_batch_edges(D, A, B):
    import torch

    learner, flat = _learner(D, A, 41)
    n_rows = 193 + 128
    obs, mask, mk, *rest = R.make_rows(D, A, n_rows, seed=B, flat=flat, masked=True)
    data = device_rows(obs, mk, *rest)
    perm = torch.randperm(n_rows, generator=torch.Generator().manual_seed(B))
    # B = 2: the largest float32 error over 64 pairs of other rows is the yardstick
    for rows, name in ((None, "rows_dev=NULL"), (perm[:B], "permuted rows_dev")):
        yard = None
        if B <= 2:
            others = torch.arange(B, B + 64 * B) if rows is None else perm[B:B + 64 * B]
            yard = others.reshape(64, B)
        check_loss_grad(D, A, flat, learner, data, rows, f"{D}->{A} B={B} {name}", yardstick_rows=yard, batch=B)


# ---- grid caps ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def many_rows():
    D, A = MONO
    flat = R.random_flat(D, A, 43)
    return flat, R.make_rows(D, A, ADV_PARTIAL_ROWS + 1025, seed=5, flat=flat, masked=True)


# with cap = min(2 CUs, 512) workgroups of two tile slots: at 128 cap rows every slot has one tile, one row more and a
# wave takes a second tile, 65 more and both slots of workgroup 0 do; at 262 144 rows k_ppo_adv_partial's grid stops
# growing and a thread's stride loop goes past its four rows
CAP_CASES = {"slabs-1": ("slabs", -1), "slabs": ("slabs", 0), "slabs+1": ("slabs", 1), "slabs+65": ("slabs", 65),
             "adv-1": ("adv", -1), "adv": ("adv", 0), "adv+1": ("adv", 1), "adv+1025": ("adv", 1025)}


@pytest.mark.parametrize("where", list(CAP_CASES))
def test_grid_caps(many_rows, where):
    import marl_sortingenv_amd as M

    D, A = MONO
    flat, (obs, mask, mk, *rest) = many_rows
    base, off = CAP_CASES[where]
    B = (128 * _slab_cap() if base == "slabs" else ADV_PARTIAL_ROWS) + off
    assert 0 < B <= obs.shape[0]
    pol, _ = make_policy(D, A, 43, precision="f32")
    learner = M.PPOLearner(pol, **HP)
    data = device_rows(obs[:B], mk[:B], *[t[:B] for t in rest])
    check_loss_grad(D, A, flat, learner, data, None, f"mono B={B} ({where}, cap {_slab_cap()})")


# ---- index semantics ------------------------------------------------------------------------------------------------------
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
    assert rows.unique().numel() < n_rows  # some rows never occur, others repeat
    check_loss_grad(D, A, flat, learner, device_rows(*cpu), rows, f"{D}->{A} repeated rows, batch = 3 n_rows")


@pytest.mark.parametrize("first", ["in range", "clamped pivot"])
@pytest.mark.parametrize("D,A", [MONO, (32, 32)])
def test_rows_outside_the_rollout_are_clamped(D, A, first):
    import torch

    n_rows = 100
    learner, flat, cpu = _index_case(D, A, n_rows, 3)
    rows = torch.randperm(n_rows, generator=torch.Generator().manual_seed(4))[:80]
    rows[[5, 17, 40, 79]] = torch.tensor([-5, n_rows, n_rows + 10 ** 9, -2 ** 62])
    if first == "clamped pivot":  # rows[0] is the pivot of the advantage statistics
        rows[0] = n_rows + 10 ** 9
    clamped = rows.clamp(0, n_rows - 1)
    ref = [t[clamped] for t in cpu]
    check_loss_grad(D, A, flat, learner, device_rows(*cpu), rows, f"{D}->{A} rows outside [0, n_rows), first {first}", ref_args=ref)


@pytest.mark.parametrize("D,A", [MONO, (32, 32), (13, 2)])
def test_actions_outside_the_head_are_clamped(D, A):
    import torch

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
    check_loss_grad(D, A, flat, learner, device_rows(obs, mk, bad, *rest), None, f"{D}->{A} actions outside [0, A)",
                    ref_args=[obs, mk, clamped, *rest])


@pytest.mark.parametrize("D,A", [MONO, (32, 32), (16, 11)])
def test_an_action_whose_mask_bit_is_zero(D, A):
    """The reference is R.forward as it is: the logit is -1e8, so is the log-probability, the ratio is 0 and approx_kl
    is of order 1e8 / B."""
    import torch

    n_rows = 300
    learner, flat, cpu = _index_case(D, A, n_rows, 7)
    obs, mk, actions, *rest = cpu
    mk = mk.clone()
    picked = [int(r) for r in torch.nonzero(actions != 0).squeeze(1)[[2, 9, 30]]]  # action 0 stays legal in every row
    for r in picked:
        mk[r, int(actions[r])] = False
    _, _, stats = check_loss_grad(D, A, flat, learner, device_rows(obs, mk, actions, *rest), None,
                                  f"{D}->{A} {len(picked)} rows with an illegal action")
    assert float(stats[4]) > 1e5  # approx_kl carries the -1e8
    # ... and its float32 error (of order 1e-2) is the largest of the eight, which check_loss_grad's one bound for all
    # statistics inherits; the others are held to the rule with approx_kl left out of the yardstick
    args = (D, A, obs, mk, actions, *rest, HP["clip_range"], HP["ent_coef"], HP["vf_coef"], True)
    s64, s32 = R.loss_and_grad(flat, torch.float64, *args)[1], R.loss_and_grad(flat, torch.float32, *args)[1]
    keep = [0, 1, 2, 3, 5, 6, 7]
    err = np.abs(stats.cpu().double().numpy() - s64.numpy())[keep]
    print(f"{D}->{A} statistics without approx_kl: err {err.max():.3e}, f32 {float((s32.double() - s64)[keep].abs().max()):.3e}")
    assert np.all(err <= R.stats_bound(s64[keep], s32[keep]))


# ---- nothing outside the outputs is written --------------------------------------------------------------------------------
@pytest.mark.parametrize("D,A", [MONO, (32, 32), (1, 1)])
def test_loss_grad_writes_its_outputs_and_nothing_else(D, A):
    import torch

    learner, flat = _learner(D, A, 53)
    obs, mask, mk, *rest = R.make_rows(D, A, 300, seed=9, flat=flat, masked=True)
    W, band, sentinel = flat.numel(), 64, 12345.0
    gbuf = torch.full((W + 2 * band,), sentinel, device="cuda")
    sbuf = torch.full((8 + 2 * band,), sentinel, device="cuda")
    gbuf[band:band + W] = float("nan")
    sbuf[band:band + 8] = float("nan")
    check_loss_grad(D, A, flat, learner, device_rows(obs, mk, *rest), None, f"{D}->{A} into banded buffers",
                    grad_out=gbuf[band:band + W], stats_out=sbuf[band:band + 8])
    for buf, n in ((gbuf, W), (sbuf, 8)):
        assert bool((buf[:band] == sentinel).all()) and bool((buf[band + n:] == sentinel).all())
        assert not bool(torch.isnan(buf[band:band + n]).any())


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
    learner, flat = _learner(D, A, 59)
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
