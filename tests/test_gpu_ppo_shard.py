"""GPU: one minibatch whose rows live in several places (mse_ppo_shard_moments, mse_ppo_shard_loss_grad, mse_ppo_shard_finish;
PPOLearner.shard_moments / shard_partial / shard_finish) and `PPOLearner(exchange=...)`.

In one process "virtual ranks" are shards of one minibatch: the test calls the phase methods for each shard and sums the
moments and the partials itself, in rank order, in double - what an all-reduce does.  The combined result of the finish is
held against the float64 autograd of tests/ppo_reference.py (tests/ppo_vclip_reference.py with old_values) on the
concatenated rows under that file's tolerance rule: R.grad_bound / R.stats_bound, 4 x torch's own float32 error, computed
each run.  The world-size-1 update over RCCL is held bit for bit against a loop of the phase methods written out by hand."""
import functools
import os
import socket

import numpy as np
import pytest

from tests import ppo_reference as R
from tests import ppo_vclip_reference as V
from tests.ppo_checks import DIMS, HP, ROWS_PER_GROUP, SLAB_CAP_OFFSETS, device_rows, group_cap, make_learner, make_policy, same_bits
from tests.test_ppo_shard_cpu import SHARD_DIMS, SPLITS

pytestmark = pytest.mark.gpu

MONO = DIMS["mono"]
FORMS = ["fma", "matrix"]
C_VF = V.GPU_C
N_ROWS = 130  # one full workgroup pass (two tiles of 64) and a 2-row tail


# ---- the virtual ranks -------------------------------------------------------------------------------------------------------------
def shards_of(data, sizes):
    """consecutive row ranges of one device dict as shards: [(data, rows i64 device tensor or None for an empty one, size)]"""
    import torch

    out, at = [], 0
    for n in sizes:
        out.append((data, torch.arange(at, at + n, device="cuda") if n > 0 else None, n))
        at += n
    return out


def run_phases(learner, shards, w_dev, stats=None, grad=None, control=None, target_kl=0.0, keep=None):
    """moments of every shard, their sum in rank order; partials of every shard on that sum, their sum in rank order; the
    finish.  -> (gradient, statistics), both device tensors.  keep: a dict that receives the per-shard results."""
    import torch

    B = sum(n for _, _, n in shards)
    ms = [learner.shard_moments(d, rows, n, control=control, out=torch.zeros(4, dtype=torch.float64, device="cuda"))
          for d, rows, n in shards]
    moments = ms[0].clone()
    for m in ms[1:]:
        moments += m
    n_partial = int(learner.L.mse_ppo_shard_partial_len(learner.policy.obs_dim, learner.policy.n_actions))
    ps = [learner.shard_partial(d, rows, n, B, moments, control=control, weights=w_dev,
                                out=torch.zeros(n_partial, dtype=torch.float64, device="cuda")) for d, rows, n in shards]
    reduced = ps[0].clone()
    for p in ps[1:]:
        reduced += p
    stats = torch.zeros(8, device="cuda") if stats is None else stats
    grad = torch.zeros(w_dev.numel(), device="cuda") if grad is None else grad
    learner.shard_finish(B, reduced, moments, stats, control=control, target_kl=target_kl, grad_out=grad)
    torch.cuda.synchronize()
    if keep is not None:
        keep.update(moments=ms, partials=ps, summed_moments=moments, reduced=reduced)
    return grad, stats


def held_to_the_yardstick(g, stats, ref, label, e32_others=0.0, allowed_others=0.0):
    import torch

    g64, s64, g32, s32 = ref
    scale, allowed = R.grad_bound(g64, g32)
    allowed = max(allowed, allowed_others)
    err = float((g.cpu().double() - g64).abs().max()) / scale
    serr = np.abs(stats.cpu().double().numpy() - s64.numpy())
    print(f"{label}: kernel grad err {err:.3e}, f32 yardstick {allowed / 4:.3e} (allowed {allowed:.3e}); "
          f"stats err {serr.max():.3e}, f32 stats err {float((s32.double() - s64).abs().max()):.3e}")
    assert torch.isfinite(g).all() and torch.isfinite(stats).all(), label
    assert err <= allowed, (label, err, allowed)
    assert np.all(serr <= R.stats_bound(s64, s32, e32_others)), (label, stats.cpu(), s64)


def reference(D, A, flat, cpu, vclip, normalize):
    """(g64, s64, g32, s32) on the CPU rows `cpu` = [obs, mk, actions, old_logp, adv, ret(, old_values)]"""
    import torch

    tail = (HP["clip_range"], HP["ent_coef"], HP["vf_coef"])
    if vclip:
        args = (D, A, *cpu, *tail, C_VF, normalize)
        return (*V.loss_and_grad(flat, torch.float64, *args), *V.loss_and_grad(flat, torch.float32, *args))
    args = (D, A, *cpu[:6], *tail, normalize)
    return (*R.loss_and_grad(flat, torch.float64, *args), *R.loss_and_grad(flat, torch.float32, *args))


@functools.lru_cache(maxsize=None)
def case(D, A, vclip, masked, normalize, n_rows=N_ROWS, seed=11):
    """one row set, its device dict and its reference, shared by both arithmetics and all splits; never modified"""
    flat = R.random_flat(D, A, D * 100 + A)
    if vclip:
        obs, mask, mk, actions, old_logp, adv, ret, old = V.make_vclip_rows(D, A, n_rows, seed, flat, masked, C_VF)
        V.assert_margins(flat, D, A, obs, mk, ret, old, C_VF)
        cpu = [obs, mk, actions, old_logp, adv, ret, old]
    else:
        obs, mask, mk, *rest = R.make_rows(D, A, n_rows, seed=seed, flat=flat, masked=masked)
        cpu = [obs, mk, *rest]
    data = device_rows(*cpu[:6])
    if vclip:
        data["values"] = cpu[6].contiguous().cuda()
    return flat, cpu, data, reference(D, A, flat, cpu, vclip, normalize)


def learner_for(D, A, arithmetic, vclip, normalize=True):
    learner, _ = make_learner(D, A, D * 100 + A, normalize=normalize, arithmetic=arithmetic)
    if vclip:
        learner.clip_range_vf = C_VF
    return learner


# ---- 1. against the float64 yardstick ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("vclip", [False, True])
@pytest.mark.parametrize("arithmetic", FORMS)
@pytest.mark.parametrize("D,A", SHARD_DIMS)
def test_every_split_against_float64(D, A, arithmetic, vclip, masked, normalize):
    flat, cpu, data, ref = case(D, A, vclip, masked, normalize)
    learner = learner_for(D, A, arithmetic, vclip, normalize)
    w = flat.cuda()
    for sizes in SPLITS:
        assert sum(sizes) == N_ROWS
        g, stats = run_phases(learner, shards_of(data, sizes), w)
        held_to_the_yardstick(g, stats, ref, f"{arithmetic} {D}->{A} vclip={vclip} masked={masked} normalize={normalize} {sizes}")
        if not normalize:
            assert stats[6:].tolist() == [0.0, 1.0]


@pytest.fixture(scope="module")
def past_the_cap():
    """a total beside ROWS_PER_GROUP * group_cap(): the large shard's first workgroup makes a second pass on both tile slots"""
    D, A = MONO
    n = ROWS_PER_GROUP * group_cap() + SLAB_CAP_OFFSETS[-1] + N_ROWS
    return (n, *case(D, A, False, True, True, n_rows=n, seed=5))


@pytest.mark.parametrize("arithmetic", FORMS)
def test_a_second_pass_of_a_workgroup(past_the_cap, arithmetic):
    D, A = MONO
    n, flat, cpu, data, ref = past_the_cap
    learner = learner_for(D, A, arithmetic, False)
    sizes = [n - N_ROWS, N_ROWS]
    assert sizes[0] == ROWS_PER_GROUP * group_cap() + 65
    g, stats = run_phases(learner, shards_of(data, sizes), flat.cuda())
    held_to_the_yardstick(g, stats, ref, f"{arithmetic} mono {sizes} (cap {group_cap()})")


# ---- 2. edges ----------------------------------------------------------------------------------------------------------------------------
def _others_yardstick(D, A, flat, cpu, B, vclip=False):
    """tests/ppo_checks.py batch_edges: with B <= 2 the float32 yardstick's error is one draw of a heavy-tailed quantity, so the
    bound takes the largest float32 error among 64 evaluations of the same size on other rows - torch alone"""
    import torch

    allowed, e32 = 0.0, 0.0
    for r in torch.arange(B, B + 64 * B).reshape(64, B):
        g64, s64, g32, s32 = reference(D, A, flat, [None if t is None else t[r] for t in cpu], vclip, True)
        allowed = max(allowed, R.grad_bound(g64, g32)[1])
        e32 = max(e32, float((s32.double() - s64).abs().max()))
    return dict(e32_others=e32, allowed_others=allowed)


@pytest.mark.parametrize("arithmetic", FORMS)
def test_global_batch_1_is_not_normalised(arithmetic):
    D, A = MONO
    flat, cpu, data, _ = case(D, A, False, True, True)
    learner = learner_for(D, A, arithmetic, False)
    assert bool(learner.params.normalize_advantage)
    g, stats = run_phases(learner, shards_of(data, [1, 0]), flat.cuda())
    ref = reference(D, A, flat, [None if t is None else t[:1] for t in cpu], False, True)
    held_to_the_yardstick(g, stats, ref, f"{arithmetic} [1, 0]", **_others_yardstick(D, A, flat, cpu, 1))
    assert stats[6:].tolist() == [0.0, 1.0]


@pytest.mark.parametrize("arithmetic", FORMS)
def test_global_batch_2_is_normalised(arithmetic):
    D, A = MONO
    flat, cpu, data, _ = case(D, A, False, True, True)
    learner = learner_for(D, A, arithmetic, False)
    g, stats = run_phases(learner, shards_of(data, [1, 1]), flat.cuda())
    ref = reference(D, A, flat, [None if t is None else t[:2] for t in cpu], False, True)
    held_to_the_yardstick(g, stats, ref, f"{arithmetic} [1, 1]", **_others_yardstick(D, A, flat, cpu, 2))
    a = cpu[4][:2].double()
    assert abs(float(stats[6]) - float(a.mean())) <= 1e-6 and abs(float(stats[7]) - float(a.std())) <= 1e-6
    assert float(stats[7]) > 0.0


@pytest.mark.parametrize("arithmetic", FORMS)
def test_rows_outside_the_rollout_are_clamped(arithmetic):
    import torch

    D, A = MONO
    flat, cpu, data, _ = case(D, A, False, True, True)
    learner = learner_for(D, A, arithmetic, False)
    rows = torch.randperm(N_ROWS, generator=torch.Generator().manual_seed(4))[:100]
    rows[[0, 5, 17, 70, 99]] = torch.tensor([N_ROWS + 10 ** 9, -5, N_ROWS, N_ROWS + 10 ** 9, -2 ** 62])
    clamped = rows.clamp(0, N_ROWS - 1)
    shards = [(data, rows[:64].cuda(), 64), (data, rows[64:].cuda(), 36)]  # a clamped index in each shard, one of them first
    g, stats = run_phases(learner, shards, flat.cuda())
    ref = reference(D, A, flat, [None if t is None else t[clamped] for t in cpu], False, True)
    held_to_the_yardstick(g, stats, ref, f"{arithmetic} rows outside [0, n_rows)")


@pytest.mark.parametrize("empty", [False, True])
@pytest.mark.parametrize("arithmetic", FORMS)
def test_rows_none_takes_the_first_rows_of_each_shards_own_rollout(arithmetic, empty):
    D, A = MONO
    flat, cpu, data, _ = case(D, A, False, True, True)
    learner = learner_for(D, A, arithmetic, False)
    # two rollouts: rows 0 .. 69 and rows 70 .. 129; each shard reads the first rows of its own with rows_dev = NULL
    halves = [[None if t is None else t[:70] for t in cpu], [None if t is None else t[70:] for t in cpu]]
    datas = [device_rows(*h) for h in halves]
    takes = [65, 0] if empty else [65, 33]
    g, stats = run_phases(learner, [(d, None, n) for d, n in zip(datas, takes)], flat.cuda())
    import torch

    ref_rows = [None if t is None else torch.cat([a[:takes[0]], b[:takes[1]]]) for t, a, b in zip(cpu, *halves)]
    held_to_the_yardstick(g, stats, reference(D, A, flat, ref_rows, False, True), f"{arithmetic} rows=None {takes}")


# ---- 3. exact properties ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vclip", [False, True])
@pytest.mark.parametrize("arithmetic", FORMS)
def test_two_runs_give_the_same_bits(arithmetic, vclip):
    import torch

    D, A = MONO
    flat, cpu, data, _ = case(D, A, vclip, True, True)
    learner = learner_for(D, A, arithmetic, vclip)
    keeps = [{}, {}]
    outs = [run_phases(learner, shards_of(data, [127, 2, 1]), flat.cuda(), keep=k) for k in keeps]
    assert same_bits(outs[0][0], outs[1][0]) and same_bits(outs[0][1], outs[1][1])
    for key in ("moments", "partials"):
        for a, b in zip(keeps[0][key], keeps[1][key]):
            assert torch.equal(a.view(torch.int64), b.view(torch.int64)), key
    # the moments are what the header says: count, sum a, sum a^2 in double, 0; the fourth cell and the padding are zero
    at = 0
    for m, n in zip(keeps[0]["moments"], [127, 2, 1]):
        a = cpu[4][at:at + n].double()
        m = m.cpu()
        assert float(m[0]) == n and float(m[3]) == 0.0
        assert abs(float(m[1]) - float(a.sum())) <= 1e-12 * n and abs(float(m[2]) - float((a * a).sum())) <= 1e-12 * n
        at += n
    W = flat.numel()
    for p in keeps[0]["partials"]:
        assert p.numel() % 4 == 0 and bool((p[W + 5:] == 0.0).all())


@pytest.mark.parametrize("arithmetic", FORMS)
def test_guard_bytes_and_the_gate(arithmetic):
    """every output inside a band of sentinels; a closed gate writes none of them and leaves the control block alone; an open
    one counts one minibatch per finish and stops exactly when (double)stats[4] > 1.5 * target_kl"""
    import torch

    D, A = MONO
    flat, cpu, data, _ = case(D, A, False, True, True)
    learner = learner_for(D, A, arithmetic, False)
    w = flat.cuda()
    W, band = flat.numel(), 64
    n_partial = int(learner.L.mse_ppo_shard_partial_len(D, A))
    rows = torch.arange(N_ROWS, device="cuda")

    def banded(n, dtype, sentinel, fill):
        buf = torch.full((n + 2 * band,), sentinel, dtype=dtype, device="cuda")
        buf[band:band + n] = fill
        return buf

    def intact(buf, n, sentinel):
        return bool((buf[:band] == sentinel).all()) and bool((buf[band + n:] == sentinel).all())

    def run(control, target_kl, fill=float("nan")):
        bufs = {"moments": banded(4, torch.float64, 12345.0, fill), "partial": banded(n_partial, torch.float64, 12345.0, fill),
                "grad": banded(W, torch.float32, 12345.0, fill), "stats": banded(8, torch.float32, 12345.0, fill)}
        view = {k: v[band:band + n] for (k, v), n in zip(bufs.items(), (4, n_partial, W, 8))}
        learner.shard_moments(data, rows, N_ROWS, control=control, out=view["moments"])
        learner.shard_partial(data, rows, N_ROWS, N_ROWS, view["moments"], control=control, weights=w, out=view["partial"])
        learner.shard_finish(N_ROWS, view["partial"], view["moments"], view["stats"], control=control, target_kl=target_kl,
                             grad_out=view["grad"])
        torch.cuda.synchronize()
        for (k, v), n in zip(bufs.items(), (4, n_partial, W, 8)):
            assert intact(v, n, 12345.0), k
        return view

    # no gate: everything is written, nothing beside it
    plain = run(None, 0.0)
    for k, v in plain.items():
        assert bool(torch.isfinite(v).all()), k
    kl = float(plain["stats"][4].double())
    assert kl > 0.0
    # an open gate that does not stop: the same bits, one minibatch counted per finish
    control = torch.zeros(2, dtype=torch.int32, device="cuda")
    for count in (1, 2):
        got = run(control, 2.0 * kl / 1.5)  # 1.5 * target_kl = 2 kl: (double)stats[4] is not above it
        assert control.tolist() == [0, count]
        for k in plain:
            assert torch.equal(got[k].view(torch.int32), plain[k].view(torch.int32)), k
    # ... and one that does: the statistics and the gradient are still written (SB3 logs the stopping minibatch)
    got = run(control, 0.5 * kl / 1.5)  # 1.5 * target_kl = kl / 2: above
    assert control.tolist() == [1, 3]
    for k in plain:
        assert torch.equal(got[k].view(torch.int32), plain[k].view(torch.int32)), k
    # target_kl <= 0: counted, never set
    control.zero_()
    run(control, 0.0)
    assert control.tolist() == [0, 1]
    # a closed gate: none of the four is written, the control block is unchanged
    control.copy_(torch.tensor([1, 7], dtype=torch.int32))
    closed = run(control, 2.0 * kl / 1.5, fill=777.0)
    assert control.tolist() == [1, 7]
    for k, v in closed.items():
        assert bool((v == 777.0).all()), k


# ---- 4. update() with an exchange at world size 1 over RCCL ----------------------------------------------------------------------------
N_ENVS, K_STEPS, EPOCHS, BS, SEED = 50, 3, 2, 64, 5
TOTAL = N_ENVS * K_STEPS  # 150 rows: minibatches of 64, 64 and 22


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _setup(exchange=None, **kw):
    import marl_sortingenv_amd as M

    pol, _ = make_policy(*MONO, 31)
    env = M.BatchedSortingEnv(kind="mono", num_envs=N_ENVS, device=0, base_seed=21, max_steps=5, noise_sorting=0.05, balesize=200,
                              auto_reset=True)
    col = M.FusedPolicyRollout(env, pol, K_STEPS, seed=22)
    return pol, col, M.PPOLearner(pol, learning_rate=1e-3, n_epochs=EPOCHS, batch_size=BS, seed=SEED, exchange=exchange, **HP, **kw)


def _image(pol):
    import ctypes as C

    from tests import policy_pack_reference as PR

    img = np.empty(PR.IMAGE_FLOATS, dtype=np.float32)
    assert pol.L.mse_policy_read_image(pol._h, C.c_void_p(img.ctypes.data)) == 0
    return img.view(np.uint32)


def _hand_loop(learner, data, target_kl):
    """update() with a world of one, written out over the phase methods and adam_step, with no collective in it"""
    import torch

    from marl_sortingenv_amd.learner import compute_gae

    compute_gae(data, learner.gamma, learner.gae_lambda)
    per_epoch = -(-TOTAL // BS)
    stats = torch.zeros((EPOCHS * per_epoch, 8), device="cuda")
    control = None if target_kl is None else torch.zeros(2, dtype=torch.int32, device="cuda")
    step0, i = learner.step, 0
    for _ in range(EPOCHS):
        if learner.shuffle == "device":
            perm = learner.permutation(TOTAL, learner.epochs_done).cuda()
            learner.epochs_done += 1
        else:
            perm = torch.randperm(TOTAL, generator=learner.generator).cuda()
        for start in range(0, TOTAL, BS):
            rows = perm[start:start + BS]
            m = learner.shard_moments(data, rows, rows.numel(), control=control)
            p = learner.shard_partial(data, rows, rows.numel(), rows.numel(), m, control=control)
            learner.shard_finish(rows.numel(), p, m, stats[i], control=control, target_kl=target_kl or 0.0)
            learner.adam_step(control)
            i += 1
    torch.cuda.synchronize()
    if control is not None:
        stopped, run = control.tolist()
        learner.step = step0 + run - (1 if stopped else 0)
    return stats, control


@pytest.mark.parametrize("gated", [False, True])
@pytest.mark.parametrize("shuffle", ["cpu", "device"])
def test_update_with_a_forced_exchange_equals_the_hand_loop(shuffle, gated):
    import torch
    import torch.distributed as dist

    from marl_sortingenv_amd.sharding import GradientExchange

    if dist.is_initialized():
        pytest.skip("a process group is already up")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    _, col, _ = _setup()
    data = {k: v.clone() for k, v in col.collect().items()}
    # a threshold inside the update: the largest approx_kl of an ungated dry run's first epoch, halved
    target_kl = None
    if gated:
        _, _, dry = _setup(shuffle=shuffle)
        dry_stats, _ = _hand_loop(dry, {k: v.clone() for k, v in data.items()}, None)
        target_kl = 0.5 * float(dry_stats[:, 4].max()) / 1.5
        assert target_kl > 0.0
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0, world_size=1, device_id=dev)
    try:
        ex = GradientExchange(device=dev, force_collective=True)
        assert ex.collective and (ex.rank, ex.world) == (0, 1)
        xpol, _, xl = _setup(exchange=ex, shuffle=shuffle, weight_sync="device", target_kl=target_kl)
        assert xl.seed == SEED and "exchange_world" in xl.hyperparameters()
        out = xl.update({k: v.clone() for k, v in data.items()})
        torch.cuda.synchronize()
        in_sync = ex.same_on_all_ranks(xl.weights)
    finally:
        dist.destroy_process_group()
    hpol, _, hl = _setup(shuffle=shuffle, weight_sync="device", target_kl=target_kl)
    assert "exchange_world" not in hl.hyperparameters() and "exchange_world" not in hl.state_dict()["hyperparameters"]
    stats, control = _hand_loop(hl, {k: v.clone() for k, v in data.items()}, target_kl)
    assert in_sync is True
    assert out["stats"].shape == stats.shape == (EPOCHS * 3, 8)
    assert same_bits(out["stats"], stats)
    for name in ("weights", "m", "v"):
        assert same_bits(getattr(xl, name), getattr(hl, name)), name
    assert xl.step == hl.step
    if gated:
        stopped, run = control.tolist()
        assert (out["stopped"], out["minibatches_run"]) == (bool(stopped), run)
        assert stopped == 1 and 0 < run <= EPOCHS * 3 and xl.step == run - 1
    else:
        assert xl.step == EPOCHS * 3 and "stopped" not in out
    # the policy's packed image after weight_sync="device" is the plain learner's repack of the same weights
    hl._hand_over()
    hl.policy.sync()
    assert np.array_equal(_image(xpol), _image(hpol))


# ---- 5. the refusals of PPOLearner(exchange=...), each by message --------------------------------------------------------------------
def test_refusals():
    import marl_sortingenv_amd as M
    from marl_sortingenv_amd.sharding import GradientExchange

    ex = GradientExchange()  # no process group: a world of one, every call a no-op
    pol, col, learner = _setup(exchange=ex)
    with pytest.raises(ValueError, match="bc_coef cannot be combined with an exchange"):
        M.PPOLearner(pol, bc_coef=0.5, exchange=ex)
    with pytest.raises(ValueError, match="ImitationLearner cannot be combined with an exchange"):
        M.ImitationLearner(pol, exchange=ex)
    with pytest.raises(ValueError, match="explained_variance=True.* cannot be combined with an exchange"):
        learner.learn(col, 1, explained_variance=True)
    with pytest.raises(ValueError, match="explained_variance cannot be combined with an exchange"):
        learner.update(col.collect(), explained_variance=True)
    _, col2, plain = _setup()
    with pytest.raises(ValueError, match="check_sync needs an exchange"):
        plain.learn(col2, 1, check_sync=True)
    kicked = M.PPOLearner(pol, bc_coef=0.5, **HP)
    with pytest.raises(ValueError, match="bc_coef has no sharded form"):
        kicked.shard_moments(col.collect(), None, 1)
    # and what is not refused: learn() with the no-op exchange, the sync check on
    hist = learner.learn(col, 2, check_sync=True)
    assert [rec["in_sync"] for rec in hist] == [True, True] and all(np.isfinite(rec["loss"]) for rec in hist)
