"""CPU checks of the data-parallel learner's pieces (no device needed): the refusals of the three shard entry points
(mse_ppo_shard_moments, mse_ppo_shard_loss_grad, mse_ppo_shard_finish) and the order they are made in, the minibatch plan,
the moments rule of include/mse.h restated in numpy, the sharded sum restated in torch float32 under the tolerance rule of
tests/ppo_reference.py, GradientExchange under gloo at world size 2, and the learner's refusals."""
import ctypes as C
import datetime
import os
import socket
import time

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import marl_sortingenv_amd as M
from marl_sortingenv_amd._lib import EXPORTS, MsePpoParams
from marl_sortingenv_amd.sharding import GradientExchange, shard_minibatch_plan
from tests import ppo_reference as R
from tests.ppo_checks import HP

INVALID, ALIGNMENT, NO_DEVICE = -1, -6, -3
# what tests/test_gpu_ppo_shard.py cuts its 130 rows into: one full workgroup pass and a 2-row tail, a shard on each side of
# the 64-row tile and of the 128-row group edge, an empty shard
SPLITS = [[130], [1, 129], [64, 66], [0, 130], [127, 2, 1]]
SHARD_DIMS = [(29, 22), (32, 32), (13, 2), (1, 1)]


# ---- 1. the C ABI refuses before any device call --------------------------------------------------------------------------------
def _params(**kw):
    f = dict(struct_size=C.sizeof(MsePpoParams), clip_range=0.2, ent_coef=0.0, vf_coef=0.5, normalize_advantage=1)
    f.update(kw)
    return MsePpoParams(f["struct_size"], f["clip_range"], f["ent_coef"], f["vf_coef"], f["normalize_advantage"])


def _harness(entry, ok):
    L = M.load_library()
    fn = getattr(L, entry)

    def call(**change):
        a = list(ok)
        for k, v in change.items():
            a[int(k[1:])] = v
        return fn(*a)

    def refused(why, status=INVALID, **change):
        assert L.mse_ppo_shuffle_host(0, 0, 0, 0, 0, None) == INVALID  # leaves another message behind
        assert call(**change) == status, (entry, change)
        err = L.mse_last_error()
        assert entry.encode() in err and why in err, (change, err)

    return L, call, refused


def test_exports_and_partial_len():
    L = M.load_library()
    for name in ("mse_ppo_shard_partial_len", "mse_ppo_shard_moments", "mse_ppo_shard_loss_grad", "mse_ppo_shard_finish"):
        assert hasattr(L, name) and name in EXPORTS
    for D, A in SHARD_DIMS + [(16, 11), (1, 32)]:
        W = int(L.mse_policy_num_weights(D, A))
        n = int(L.mse_ppo_shard_partial_len(D, A))
        assert n % 4 == 0 and W + 5 <= n < W + 5 + 4  # W gradient sums, five statistic sums, padding to a multiple of 4
        # the slabs the partial is summed from fit the workspace the learner already owns
        assert 8 * n <= L.mse_ppo_workspace_bytes(D, A)
    assert L.mse_ppo_shard_partial_len(0, 2) == 0 and L.mse_ppo_shard_partial_len(29, 33) == 0
    assert L.mse_ppo_workspace_bytes(1, 1) >= 256 * 2 * 8  # the moments' partial pairs


def test_moments_checks_its_arguments_before_any_device_call():
    one = C.c_void_p(16)
    #      0 n_rows, 1 rows, 2 batch_local, 3 advantages, 4 moments_out, 5 workspace, 6 stream, 7 control
    ok = [64, None, 64, one, one, one, None, None]
    L, call, refused = _harness("mse_ppo_shard_moments", ok)
    for i in (3, 4, 5):
        refused(b"null", **{f"a{i}": None})
    refused(b"batch_local", a2=-1)
    refused(b"batch_local", a2=65)  # batch_local > n_rows without rows_dev
    refused(b"batch_local", a0=0)
    for off in (8, 4, 1):
        refused(b"workspace must be 16-byte aligned", status=ALIGNMENT, a5=C.c_void_p(16 + off))
    for off in (4, 1):
        refused(b"moments_out must be 8-byte aligned", status=ALIGNMENT, a4=C.c_void_p(16 + off))
    # the documented order: null, the row counts, the workspace, moments_out
    refused(b"null", a3=None, a2=-1)
    refused(b"batch_local", a2=-1, a5=C.c_void_p(24))
    refused(b"workspace", status=ALIGNMENT, a5=C.c_void_p(24), a4=C.c_void_p(20))
    if torch.cuda.is_available():
        return  # with a device the well-formed call would follow the pointers
    assert call() == NO_DEVICE and b"no HIP device" in L.mse_last_error()
    assert call(a2=0, a1=None) == NO_DEVICE  # an empty shard is legal
    assert call(a2=1000, a1=one) == NO_DEVICE  # with rows_dev batch_local may exceed n_rows
    assert call(a7=one) == NO_DEVICE


def test_loss_grad_checks_its_arguments_before_any_device_call():
    one = C.c_void_p(16)
    p = _params()
    #      0 D, 1 A, 2 weights, 3 n_rows, 4 rows, 5 batch_local, 6 obs, 7 mask, 8 actions, 9 old_logp, 10 adv, 11 ret, 12 params,
    #      13 global_batch, 14 moments, 15 partial_out, 16 workspace, 17 stream, 18 control, 19 arithmetic, 20 old_values, 21 c_vf
    ok = [29, 22, one, 64, None, 64, one, None, one, one, one, one, C.byref(p), 100, one, one, one, None, None, 0, one, 0.2]
    L, call, refused = _harness("mse_ppo_shard_loss_grad", ok)
    for i in (2, 6, 8, 9, 10, 11, 12, 14, 15, 16):
        refused(b"null", **{f"a{i}": None})
    for D, A in ((0, 22), (33, 22), (29, 0), (29, 33), (-1, 1)):
        refused(b"1..32", a0=D, a1=A)
    for size in (0, 3, C.sizeof(MsePpoParams) - 4, C.sizeof(MsePpoParams) + 4):
        bad = _params(struct_size=size)
        refused(b"struct_size", a12=C.byref(bad))
    refused(b"batch_local", a5=-1)
    refused(b"batch_local", a5=65, a13=65)  # batch_local > n_rows without rows_dev
    refused(b"batch_local", a3=0)
    for b_local, b_global in ((64, 63), (64, 0), (0, 0), (0, -1), (1, 0)):
        refused(b"global_batch", a5=b_local, a13=b_global)
    nan = _params(clip_range=float("nan"))
    refused(b"clip_range /", a12=C.byref(nan))
    for off in (8, 4, 1):
        refused(b"workspace must be 16-byte aligned", status=ALIGNMENT, a16=C.c_void_p(16 + off))
    for i in (14, 15):
        refused(b"8-byte aligned", status=ALIGNMENT, **{f"a{i}": C.c_void_p(20)})
    for arithmetic in (-1, 2):
        refused(b"arithmetic", a19=arithmetic)
        refused(b"arithmetic", a19=arithmetic, a20=None)
    for c in (0.0, -0.1, float("nan"), float("inf"), float("-inf"), 1e-60):
        for arithmetic in (0, 1):
            refused(b"clip_range_vf", a21=c, a19=arithmetic)
    # the documented order
    bad = _params(struct_size=3, clip_range=float("nan"))
    refused(b"null", a2=None, a0=0)
    refused(b"1..32", a0=0, a12=C.byref(bad))
    refused(b"struct_size", a12=C.byref(bad), a5=-1)
    refused(b"batch_local", a5=-1, a13=0)
    refused(b"global_batch", a13=63, a12=C.byref(nan))
    refused(b"clip_range /", a12=C.byref(nan), a16=C.c_void_p(24))
    refused(b"workspace", status=ALIGNMENT, a16=C.c_void_p(24), a14=C.c_void_p(20))
    refused(b"8-byte aligned", status=ALIGNMENT, a14=C.c_void_p(20), a19=2)
    refused(b"arithmetic", a19=2, a21=0.0)
    if torch.cuda.is_available():
        return
    for arithmetic in (0, 1):
        assert call(a19=arithmetic) == NO_DEVICE and b"no HIP device" in L.mse_last_error()
        assert call(a19=arithmetic, a20=None, a21=float("nan")) == NO_DEVICE  # without old_values clip_range_vf is not read
        assert call(a19=arithmetic, a5=0, a4=None) == NO_DEVICE  # an empty shard is legal
        assert call(a19=arithmetic, a13=64, a18=one) == NO_DEVICE  # global_batch == batch_local: a world of one


def test_finish_checks_its_arguments_before_any_device_call():
    one = C.c_void_p(16)
    p = _params()
    #      0 D, 1 A, 2 global_batch, 3 reduced, 4 moments, 5 params, 6 grad_out, 7 stats_out, 8 stream, 9 target_kl, 10 control
    ok = [29, 22, 100, one, one, C.byref(p), one, one, None, 0.01, None]
    L, call, refused = _harness("mse_ppo_shard_finish", ok)
    refused(b"target_kl", a9=float("nan"), a10=one)
    for i in (3, 4, 5, 6, 7):
        refused(b"null", **{f"a{i}": None})
    for D, A in ((0, 22), (33, 22), (29, 0), (29, 33)):
        refused(b"1..32", a0=D, a1=A)
    for size in (0, C.sizeof(MsePpoParams) + 4):
        bad = _params(struct_size=size)
        refused(b"struct_size", a5=C.byref(bad))
    for b in (0, -1):
        refused(b"global_batch", a2=b)
    inf = _params(ent_coef=float("inf"))
    refused(b"ent_coef", a5=C.byref(inf))
    for i in (3, 4):
        refused(b"8-byte aligned", status=ALIGNMENT, **{f"a{i}": C.c_void_p(20)})
    # the documented order
    bad = _params(struct_size=3, ent_coef=float("inf"))
    refused(b"target_kl", a9=float("nan"), a10=one, a3=None)
    refused(b"null", a3=None, a0=0)
    refused(b"1..32", a0=0, a5=C.byref(bad))
    refused(b"struct_size", a5=C.byref(bad), a2=0)
    refused(b"global_batch", a2=0, a5=C.byref(inf))
    refused(b"ent_coef", a5=C.byref(inf), a3=C.c_void_p(20))
    if torch.cuda.is_available():
        return
    assert call() == NO_DEVICE and b"no HIP device" in L.mse_last_error()
    assert call(a9=float("nan")) == NO_DEVICE  # without a control block target_kl is not read
    assert call(a10=one) == NO_DEVICE


# ---- 2. the minibatch plan ------------------------------------------------------------------------------------------------------
def test_shard_minibatch_plan():
    assert shard_minibatch_plan([64, 64], 16) == [[16, 16]] * 4
    # ragged: totals 50 and 45 at 16 rows per rank -> rank 0 meets [16, 16, 16, 2], rank 1 [16, 16, 13, 0]
    plan = shard_minibatch_plan([50, 45], 16)
    assert plan == [[16, 16], [16, 16], [16, 13], [2, 0]]
    assert [m[0] for m in plan] == [16, 16, 16, 2] and [m[1] for m in plan] == [16, 16, 13, 0]
    assert [sum(m) for m in plan] == [32, 32, 29, 2]  # the global batches
    # a rank with fewer rows than one batch: it is in the first minibatch only, and short there
    assert shard_minibatch_plan([40, 5, 33], 16) == [[16, 5, 16], [16, 0, 16], [8, 0, 1]]
    assert shard_minibatch_plan([40, 0], 16) == [[16, 0], [16, 0], [8, 0]]
    # batch_size >= every total: one minibatch of everything
    assert shard_minibatch_plan([50, 45], 50) == [[50, 45]] and shard_minibatch_plan([50, 45], 10 ** 9) == [[50, 45]]
    assert shard_minibatch_plan([150], 64) == [[64], [64], [22]]  # a world of one: update()'s own cut
    rng = np.random.default_rng(0)
    for _ in range(200):
        totals = [int(t) for t in rng.integers(0, 300, size=int(rng.integers(1, 6)))]
        totals[int(rng.integers(len(totals)))] += 1
        bs = int(rng.integers(1, 350))
        plan = shard_minibatch_plan(totals, bs)
        assert len(plan) == -(-max(totals) // bs)
        assert [sum(m[r] for m in plan) for r in range(len(totals))] == totals  # every row once per epoch
        for r, t in enumerate(totals):  # rank r's j-th minibatch is rows [j bs, min((j + 1) bs, t)) of its permutation
            assert [m[r] for m in plan] == [max(0, min((j + 1) * bs, t) - j * bs) for j in range(len(plan))]
        assert all(sum(m) >= 1 for m in plan)  # the rank with the most rows is in every minibatch
    for bad in (([], 16), ([0, 0], 16), ([5, -1], 16), ([5], 0)):
        with pytest.raises(ValueError):
            shard_minibatch_plan(*bad)


# ---- 3. the moments rule of include/mse.h, restated --------------------------------------------------------------------------------
def moments_of(piece):
    """mse_ppo_shard_moments of one shard: {count, sum a, sum a^2, 0} in double"""
    a = piece.astype(np.float64)
    return np.array([a.size, a.sum(), (a * a).sum(), 0.0])


def mean_std_from(moments, B):
    """the header's sentence: mean = sum a / B; unbiased variance = (sum a^2 - (sum a)^2 / B) / (B - 1) in double, clamped
    at 0; mean and std rounded to float32 once"""
    s, q = moments[1], moments[2]
    var = (q - s * s / B) / (B - 1)
    return np.float32(s / B), np.float32(np.sqrt(max(var, 0.0)))


@pytest.mark.parametrize("sizes", [[77, 53], [130, 0], [0, 1, 129], [127, 2, 1], [1, 1], [40000, 0, 25601]])
def test_moments_rule_against_numpy(sizes):
    rng = np.random.default_rng(sum(sizes))
    adv = (rng.standard_normal(sum(sizes)) * 1.5 + 0.3).astype(np.float32)  # tests/ppo_reference.py's advantages
    pieces = np.split(adv, np.cumsum(sizes)[:-1])
    assert [p.size for p in pieces] == sizes
    total = sum(moments_of(p) for p in pieces)
    assert total[0] == adv.size and total[3] == 0.0
    mean, std = mean_std_from(total, adv.size)
    want_mean, want_std = adv.astype(np.float64).mean(), adv.astype(np.float64).std(ddof=1)
    # both sides are double-precision results (relative error of order B 2^-53, times (mean^2 + var) / var < 2 for the
    # variance's cancellation) rounded to float32 once: they are at most one float32 ulp apart
    assert abs(float(mean) - want_mean) <= np.spacing(np.float32(abs(want_mean)))
    assert abs(float(std) - want_std) <= np.spacing(np.float32(want_std))
    # the order of the pieces changes the double sums by rounding only
    again = sum(moments_of(p) for p in reversed(pieces))
    assert np.allclose(again, total, rtol=1e-13, atol=0.0)


def test_moments_rule_clamps_a_negative_variance():
    a = np.full(1000, np.float32(0.1))
    mean, std = mean_std_from(moments_of(a), a.size)
    assert mean == np.float32(0.1) and 0.0 <= std < 1e-7


# ---- 4. the sharded sum in torch float32 satisfies the yardstick's own bound --------------------------------------------------------
def sharded_loss_and_grad(flat, dtype, D, A, rows, sizes, normalize):
    """What the three phases compute, by torch alone: global moments in double, every shard's per-row terms scaled by
    1 / B, the shards' gradients added in rank order."""
    obs, mk, actions, old_logp, adv, ret = rows
    B = obs.shape[0]
    if normalize and B > 1:
        mean, std = mean_std_from(sum(moments_of(p) for p in np.split(adv.numpy(), np.cumsum(sizes)[:-1])), B)
        adv = ((adv - float(mean)) / (float(std) + 1e-8)).float()
    g, at = torch.zeros(flat.numel(), dtype=dtype), 0
    for n in sizes:
        if n > 0:
            w = flat.detach().to(dtype).clone().requires_grad_(True)
            sel = [None if t is None else t[at:at + n] for t in (obs, mk, actions, old_logp, adv, ret)]
            loss, _ = R.ppo_loss(w, D, A, *sel, HP["clip_range"], HP["ent_coef"], HP["vf_coef"], normalize=False)
            (loss * (n / B)).backward()  # a mean over n rows -> the shard's share of the mean over B
            g += w.grad
        at += n
    return g


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("D,A", SHARD_DIMS)
def test_the_reference_satisfies_its_own_bound_on_the_gpu_cases(D, A, masked, normalize):
    flat = R.random_flat(D, A, D * 100 + A)
    obs, mask, mk, *rest = R.make_rows(D, A, 130, seed=11, flat=flat, masked=masked)
    rows = (obs, mk, *rest)
    args = (D, A, *rows, HP["clip_range"], HP["ent_coef"], HP["vf_coef"], normalize)
    g64, s64 = R.loss_and_grad(flat, torch.float64, *args)
    g32, s32 = R.loss_and_grad(flat, torch.float32, *args)
    scale, allowed = R.grad_bound(g64, g32)
    assert scale > 0.0 and 0.0 < allowed < 1e-4 and torch.isfinite(g64).all()  # a bound that binds
    assert np.all(R.stats_bound(s64, s32) < 1e-4)
    for sizes in SPLITS:
        g = sharded_loss_and_grad(flat, torch.float32, D, A, rows, sizes, normalize)
        err = float((g.double() - g64).abs().max()) / scale
        assert err <= allowed, (sizes, err, allowed)


# ---- 5. GradientExchange under gloo, world size 2 ----------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _exchange_worker(rank, world, port, ok):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    try:
        ex = GradientExchange(device=torch.device("cpu"))
        assert (ex.rank, ex.world, ex.collective) == (rank, world, True)
        # all_reduce_sum, in place; rank 1 contributes zeros (an empty shard)
        mine = torch.tensor([64.0, 0.1, 1e-30, 0.0], dtype=torch.float64) if rank == 0 else torch.zeros(4, dtype=torch.float64)
        out = ex.all_reduce_sum(mine)
        assert out is mine and torch.equal(mine, torch.tensor([64.0, 0.1, 1e-30, 0.0], dtype=torch.float64))
        both = torch.arange(5, dtype=torch.float64) * (rank + 1) + 0.25
        assert torch.equal(ex.all_reduce_sum(both), torch.arange(5, dtype=torch.float64) * 3 + 0.5)
        f32 = torch.full((3,), float(rank + 1), dtype=torch.float32)
        assert torch.equal(ex.all_reduce_sum(f32), torch.full((3,), 3.0))
        with pytest.raises(ValueError):
            ex.all_reduce_sum(torch.zeros(2, dtype=torch.int32))
        # broadcast
        w = torch.arange(7, dtype=torch.float32) + 100.0 * rank
        assert torch.equal(ex.broadcast(w), torch.arange(7, dtype=torch.float32))
        w = torch.arange(7, dtype=torch.float32) + 100.0 * rank
        assert torch.equal(ex.broadcast(w, src=1), torch.arange(7, dtype=torch.float32) + 100.0)
        assert ex.all_gather_ints(50 - 5 * rank) == [50, 45]
        # same_on_all_ranks: equal bits, then one flipped bit on one rank; a NaN payload and -0.0 are bits too
        t = torch.tensor([1.5, -0.0, float("nan"), 3e-41], dtype=torch.float32)
        assert ex.same_on_all_ranks(t) is True
        if rank == 1:
            t.view(torch.int32)[3] ^= 1
        assert ex.same_on_all_ranks(t) is False
        z = torch.tensor([0.0 if rank == 0 else -0.0], dtype=torch.float32)
        assert ex.same_on_all_ranks(z) is False
        # the learner refuses what has no sharded form before it touches the policy or the exchange
        with pytest.raises(ValueError, match="bc_coef"):
            M.PPOLearner(object(), bc_coef=0.5, exchange=ex)
        with pytest.raises(ValueError, match="ImitationLearner"):
            M.ImitationLearner(object(), exchange=ex)
        ok[rank] = 1
    finally:
        dist.destroy_process_group()


def test_gradient_exchange_gloo_world_2():
    world = 2
    ok = mp.get_context("spawn").Array("i", [0] * world)
    ctx = mp.spawn(_exchange_worker, args=(world, _free_port(), ok), nprocs=world, join=False)
    deadline = time.monotonic() + 120.0
    try:
        while not ctx.join(timeout=5.0):
            if time.monotonic() > deadline:
                raise AssertionError("the gloo workers did not finish in time")
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()
    assert list(ok) == [1] * world


def test_gradient_exchange_is_a_no_op_at_world_size_1():
    assert not dist.is_initialized()
    ex = GradientExchange(force_collective=True)  # no process group: nothing to force
    assert (ex.rank, ex.world, ex.collective) == (0, 1, False)
    t = torch.tensor([1.0, 2.0], dtype=torch.float64)
    assert ex.all_reduce_sum(t) is t and ex.broadcast(t) is t and t.tolist() == [1.0, 2.0]
    assert ex.same_on_all_ranks(t.float()) is True and ex.all_gather_ints(7) == [7]


# ---- 6. the learner's refusals, by name, without a device ----------------------------------------------------------------------------
def test_learner_refusals_without_a_device():
    ex = GradientExchange()
    with pytest.raises(ValueError, match="bc_coef cannot be combined with an exchange"):
        M.PPOLearner(object(), bc_coef=0.5, exchange=ex)
    with pytest.raises(ValueError, match="ImitationLearner cannot be combined with an exchange"):
        M.ImitationLearner(object(), exchange=ex)
