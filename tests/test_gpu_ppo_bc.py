"""GPU: PPO with an auxiliary imitation term - mse_ppo_bc_loss_grad (the KICK entries of k_ppo_grad and k_ppo_grad_matrix and
the twelve-column form of the reduction) and PPOLearner(bc_coef=...).

The gradient and the statistics are held against the float64 autograd of tests/ppo_bc_reference.py under the tolerance rule
of tests/ppo_reference.py (4 x torch's own float32 error, computed each run; hits and unusable rows exactly), one reference
per case shared by both arithmetics.  With bc_coef = 0 the call must give mse_ppo_loss_grad_vclip's bits."""
import ctypes as C

import numpy as np
import pytest

from tests import ppo_bc_reference as K
from tests import ppo_reference as R
from tests.ppo_checks import DIM_MATRIX, HP, ROWS_PER_GROUP, group_cap, make_policy, same_bits

pytestmark = pytest.mark.gpu

MONO = (29, 22)
FORMS = ["fma", "matrix"]
N_ROWS = 364  # five full tiles and a 44-row tail; three workgroups
BATCHES = [1, 63, 64, 65, 128, 129, 300]


def kick_learner(D, A, seed, arithmetic, bc_coef, with_old=False, normalize=True):
    import marl_sortingenv_amd as M

    pol, flat = make_policy(D, A, seed, precision="f32")
    learner = M.PPOLearner(pol, normalize_advantage=normalize, arithmetic=arithmetic, bc_coef=bc_coef,
                           clip_range_vf=K.C_VF if with_old else None, **HP)
    assert learner.workspace.numel() == learner.L.mse_ppo_bc_workspace_bytes(D, A)
    return learner, flat


def device_data(rows):
    import torch

    d = {"observations": rows["obs"].contiguous().cuda(), "actions": rows["actions"].int().contiguous().cuda(),
         "log_probs": rows["old_logp"].contiguous().cuda(), "advantages": rows["adv"].contiguous().cuda(),
         "returns": rows["ret"].contiguous().cuda(), "expert_actions": rows["labels"].int().contiguous().cuda()}
    if rows["mk"] is not None:
        d["action_masks"] = rows["mk"].to(dtype=torch.uint8).contiguous().cuda()
    if rows["old"] is not None:
        d["values"] = rows["old"].contiguous().cuda()
    return d


def both_forms(D, A, seed, rows, idx, batch, bc_coef, label, others=None, grad_out=None, stats_out=None, learners=None):
    """one loss_grad per arithmetic on rows `idx` (None: rows 0 .. batch - 1, rows_dev = NULL), each twice (bit-equal),
    both against ONE float64 reference, then against each other -> {arithmetic: (grad, stats)} on the CPU"""
    import torch

    with_old = rows["old"] is not None
    data = device_data(rows)
    picked = K.take(rows, torch.arange(batch) if idx is None else idx.clamp(0, rows["obs"].shape[0] - 1))
    ref = None
    out = {}
    for arithmetic in FORMS:
        learner, flat = learners[arithmetic] if learners else kick_learner(D, A, seed, arithmetic, bc_coef, with_old)
        if ref is None:
            ref = K.reference(flat, D, A, picked, bc_coef, others=others)
        w = flat.cuda()
        rows_dev = None if idx is None else idx.cuda()
        stats = torch.zeros(12, device="cuda") if stats_out is None else stats_out
        g = learner.loss_grad(data, rows_dev, batch, stats, weights=w, grad_out=grad_out).clone()
        stats = stats.clone()
        stats2 = torch.zeros(12, device="cuda")
        g2 = learner.loss_grad(data, rows_dev, batch, stats2, weights=w, grad_out=torch.zeros_like(g))
        torch.cuda.synchronize()
        assert same_bits(g, g2) and same_bits(stats, stats2), "two calls with the same inputs must agree bit for bit"
        K.check(f"{arithmetic} {label}", g.cpu(), stats.cpu(), ref)
        out[arithmetic] = (g.cpu(), stats.cpu())
    (g0, s0), (g1, s1) = out["fma"], out["matrix"]
    scale, allowed = ref[3], ref[4]
    assert float((g0.double() - g1.double()).abs().max()) / scale <= 2.0 * allowed  # each is within `allowed` of float64
    assert s0[9:].tolist() == s1[9:].tolist()  # the counts
    return out


# ---- 1. both arithmetics against float64 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_old", [False, True])
@pytest.mark.parametrize("D,A", DIM_MATRIX)
def test_every_shape_at_the_tile_and_group_edges(D, A, with_old):
    import torch

    flat = R.random_flat(D, A, D * 100 + A)
    rows = K.make_kick_rows(D, A, N_ROWS, 11, flat, True, with_old)
    K.assert_margins(flat, D, A, rows)
    perm = torch.randperm(N_ROWS, generator=torch.Generator().manual_seed(7))
    learners = {f: kick_learner(D, A, D * 100 + A, f, 0.5, with_old) for f in FORMS}
    for n, B in enumerate(BATCHES):
        idx = perm[:B] if n % 2 else None  # rows_dev = NULL and a permuted rows_dev in turn
        others = None
        if B == 1:  # tests/ppo_checks.py batch_edges: the largest float32 error over 64 evaluations on other rows
            others = [K.take(rows, torch.tensor([r])) for r in range(1, 65)]
        out = both_forms(D, A, D * 100 + A, rows, idx, B, 0.5, f"{D}->{A} old_values={with_old} B={B}", others=others,
                         learners=learners)
    if A > 1:
        s = out["fma"][1]
        assert 0.3 < float(s[9]) < 1.0 and float(s[10]) > 0.0  # hits, misses and unusable rows all occur at B = 300


@pytest.mark.parametrize("D,A", [(13, 2), (16, 11), MONO, (32, 32)])
def test_unmasked(D, A):
    flat = R.random_flat(D, A, 61)
    rows = K.make_kick_rows(D, A, 300, 37, flat, False)
    K.assert_margins(flat, D, A, rows)
    for g, s in both_forms(D, A, 61, rows, None, 300, 4.0, f"{D}->{A} unmasked").values():
        assert float(s[10]) == 0.0 and 0.3 < float(s[9]) < 1.0


def test_grid_cap_second_pass():
    """128 * group_cap() + 1 rows: the first wave of workgroup 0 takes a second tile with its seven sums carried over"""
    D, A = 4, 3
    n = ROWS_PER_GROUP * group_cap() + 1
    flat = R.random_flat(D, A, 43)
    rows = K.make_kick_rows(D, A, n, 5, flat, True)
    both_forms(D, A, 43, rows, None, n, 0.5, f"4->3 B={n} (cap {group_cap()})")


def test_rows_may_repeat_and_rows_outside_are_clamped():
    import torch

    D, A = MONO
    n_rows = 100
    flat = R.random_flat(D, A, 47)
    rows = K.make_kick_rows(D, A, n_rows, 1, flat, True, True)
    idx = torch.randint(0, n_rows, (3 * n_rows,), generator=torch.Generator().manual_seed(2))
    idx[:4] = 7
    assert idx.unique().numel() < n_rows  # some rows never occur, others repeat
    both_forms(D, A, 47, rows, idx, idx.numel(), 0.5, "repeated rows, batch = 3 n_rows")
    idx = torch.randperm(n_rows, generator=torch.Generator().manual_seed(4))[:80]
    idx[[0, 5, 17, 40, 79]] = torch.tensor([n_rows + 10 ** 9, -5, n_rows, n_rows + 10 ** 9, -2 ** 62])  # [0]: the pivot
    both_forms(D, A, 47, rows, idx, 80, 0.5, "rows outside [0, n_rows)")  # both_forms clamps for the reference


def test_writes_its_outputs_and_nothing_else():
    import torch

    D, A = MONO
    flat = R.random_flat(D, A, 53)
    rows = K.make_kick_rows(D, A, 300, 9, flat, True, True)
    W, band, sentinel = flat.numel(), 64, 12345.0
    learners = {f: kick_learner(D, A, 53, f, 0.5, True) for f in FORMS}
    ws_bytes = learners["fma"][0].workspace.numel()
    for f in FORMS:  # the workspace between two guard bands (64 floats keep its 16-byte alignment)
        wbuf = torch.full((ws_bytes // 4 + 2 * band,), sentinel, device="cuda")
        learners[f][0].workspace = wbuf[band:band + ws_bytes // 4].view(torch.uint8)
        assert learners[f][0].workspace.data_ptr() % 16 == 0
        learners[f] = (*learners[f], wbuf)
    gbuf = torch.full((W + 2 * band,), sentinel, device="cuda")
    sbuf = torch.full((12 + 2 * band,), sentinel, device="cuda")
    gbuf[band:band + W] = float("nan")
    sbuf[band:band + 12] = float("nan")
    both_forms(D, A, 53, rows, None, 300, 0.5, "into banded buffers", grad_out=gbuf[band:band + W], stats_out=sbuf[band:band + 12],
               learners={f: v[:2] for f, v in learners.items()})
    for buf, n in ((gbuf, W), (sbuf, 12), (learners["fma"][2], ws_bytes // 4), (learners["matrix"][2], ws_bytes // 4)):
        assert bool((buf[:band] == sentinel).all()) and bool((buf[band + n:] == sentinel).all())
    assert int(torch.isfinite(gbuf[band:band + W]).sum()) == W and int(torch.isfinite(sbuf[band:band + 12]).sum()) == 12


# ---- 2. bc_coef = 0 is the PPO call, bit for bit; the gate -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    D, A = MONO
    flat = R.random_flat(D, A, 53)
    rows = K.make_kick_rows(D, A, 300, 9, flat, True, True)
    return flat, rows, device_data(rows)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _raw(learner, data, flat_dev, entry, tail, n_stats, fill=0.0):
    """one raw call of `entry` on rows 0 .. 299 with `tail` behind mse_ppo_loss_grad's 17 arguments -> (grad, stats)"""
    import torch

    D, A = MONO
    g = torch.full((flat_dev.numel(),), fill, device="cuda")
    s = torch.full((n_stats,), fill, device="cuda")
    args = (D, A, _ptr(flat_dev), 300, None, 300, _ptr(data["observations"]), _ptr(data["action_masks"]), _ptr(data["actions"]),
            _ptr(data["log_probs"]), _ptr(data["advantages"]), _ptr(data["returns"]), C.byref(learner.params), _ptr(g), _ptr(s),
            _ptr(learner.workspace), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert getattr(learner.L, entry)(*args, *tail) == 0, learner.L.mse_last_error()
    torch.cuda.synchronize()
    return g, s


@pytest.mark.parametrize("gated", [False, True])
@pytest.mark.parametrize("with_old", [False, True])
@pytest.mark.parametrize("arithmetic", FORMS)
def test_bc_coef_zero_gives_the_bits_of_the_ppo_call(small, arithmetic, with_old, gated):
    """the sharpest test: any change to the PPO arithmetic on the new path fails it.  torch.equal: up to the sign of a zero"""
    import torch

    flat, rows, data = small
    learner, _ = kick_learner(*MONO, 53, arithmetic, 0.0, with_old)
    w = flat.cuda()
    code = FORMS.index(arithmetic)
    controls = [torch.zeros(2, dtype=torch.int32, device="cuda") for _ in range(2)] if gated else [None, None]
    old = _ptr(data["values"]) if with_old else None
    want = _raw(learner, data, w, "mse_ppo_loss_grad_vclip", (0.01, _ptr(controls[0]), code, old, K.C_VF), 8)
    got = _raw(learner, data, w, "mse_ppo_bc_loss_grad", (0.01, _ptr(controls[1]), code, old, K.C_VF, _ptr(data["expert_actions"]), 0.0), 12)
    assert bool(torch.isfinite(want[0]).all()) and float(want[0].abs().max()) > 0.0
    assert torch.equal(got[0], want[0]) and torch.equal(got[1][:8], want[1])
    assert float(got[1][8]) > 0.0 and 0.0 < float(got[1][9]) < 1.0 and float(got[1][10]) > 0.0 and float(got[1][11]) == 0.0
    if gated:
        assert controls[0].tolist() == controls[1].tolist() and controls[0][1].item() == 1
    # ... and a coefficient moves the actor's gradient and the loss, and nothing else of the eight
    on = _raw(learner, data, w, "mse_ppo_bc_loss_grad", (0.0, None, code, old, K.C_VF, _ptr(data["expert_actions"]), 0.5), 12)
    vf_w1 = 32 * MONO[0] + 32 + 32 * 32 + 32 + MONO[1] * 32 + MONO[1]  # where the critic starts
    assert same_bits(on[0][vf_w1:], got[0][vf_w1:]) and not torch.equal(on[0][:vf_w1], got[0][:vf_w1])
    assert same_bits(on[1][1:], got[1][1:]) and float(on[1][0]) != float(got[1][0])


@pytest.mark.parametrize("arithmetic", FORMS)
def test_gate(small, arithmetic):
    import torch

    flat, rows, data = small
    learner, _ = kick_learner(*MONO, 53, arithmetic, 0.5, True)
    plain, _ = kick_learner(*MONO, 53, arithmetic, 0.5, True)
    w = flat.cuda()
    code = FORMS.index(arithmetic)
    nan = float("nan")
    tail = (code, _ptr(data["values"]), K.C_VF)
    kick = (_ptr(data["expert_actions"]), 0.5)
    g0, s0 = _raw(learner, data, w, "mse_ppo_bc_loss_grad", (0.0, None, *tail, *kick), 12, fill=nan)  # the ungated dry run
    kl = float(s0[4])
    assert kl > 0.0 and bool(torch.isfinite(g0).all()) and bool(torch.isfinite(s0).all())
    # closed on entry: neither output is written, the block is unchanged
    control = torch.tensor([1, 5], dtype=torch.int32, device="cuda")
    g, s = _raw(learner, data, w, "mse_ppo_bc_loss_grad", (1e9, _ptr(control), *tail, *kick), 12, fill=nan)
    assert control.tolist() == [1, 5]
    assert bool(torch.isnan(g).all()) and bool(torch.isnan(s).all())
    # open: the stop decision is the plain call's on either side of this minibatch's approx_kl (the gate reads [4], which the
    # imitation term does not enter)
    for target, stopped in ((0.5 * kl / 1.5, 1), (2.0 * kl / 1.5, 0)):
        control = torch.zeros(2, dtype=torch.int32, device="cuda")
        control_plain = torch.zeros(2, dtype=torch.int32, device="cuda")
        g, s = _raw(learner, data, w, "mse_ppo_bc_loss_grad", (target, _ptr(control), *tail, *kick), 12, fill=nan)
        _raw(plain, data, w, "mse_ppo_loss_grad_vclip", (target, _ptr(control_plain), *tail), 8, fill=nan)
        assert control.tolist() == control_plain.tolist() == [stopped, 1] and same_bits(g, g0) and same_bits(s, s0)
    # through the learner
    control = torch.zeros(2, dtype=torch.int32, device="cuda")
    s = torch.full((12,), nan, device="cuda")
    g = learner.loss_grad(data, None, 300, s, weights=w, grad_out=torch.full_like(g0, nan), control=control, target_kl=2.0 * kl / 1.5)
    torch.cuda.synchronize()
    assert control.tolist() == [0, 1] and same_bits(g, g0) and same_bits(s, s0)


def test_the_learner_refuses_missing_or_misshapen_labels(small):
    import torch

    flat, rows, data = small
    learner, _ = kick_learner(*MONO, 53, "fma", 0.5)
    stats = torch.zeros(12, device="cuda")
    for bad in (None, data["expert_actions"].long(), data["expert_actions"][:-1], data["expert_actions"].cpu(),
                torch.stack([data["expert_actions"]] * 2, dim=1)[:, 0]):
        d = dict(data)
        if bad is None:
            del d["expert_actions"]
        else:
            d["expert_actions"] = bad
        with pytest.raises(ValueError, match="expert_labels=True"):
            learner.loss_grad(d, None, 300, stats)


# ---- 3. update() and learn() --------------------------------------------------------------------------------------------------------
N_ENVS, K_STEPS, EPOCHS, BS, SEED = 64, 8, 2, 128, 5
TOTAL = N_ENVS * K_STEPS


def _setup(arithmetic="fma", **kw):
    import marl_sortingenv_amd as M

    pol, flat = make_policy(*MONO, 31)
    env = M.BatchedSortingEnv(kind="mono", num_envs=N_ENVS, device=0, base_seed=21, max_steps=5, noise_sorting=0.05, balesize=200,
                              auto_reset=True)
    col = M.PolicyRolloutCollector(env, pol, K_STEPS, seed=22, expert_labels=True)
    kw = {**HP, "learning_rate": 1e-3, **kw}
    learner = M.PPOLearner(pol, n_epochs=EPOCHS, batch_size=BS, seed=SEED, arithmetic=arithmetic, **kw)
    return pol, flat, col, learner


@pytest.mark.parametrize("arithmetic", FORMS)
@pytest.mark.parametrize("weight_sync", ["host", "device"])
@pytest.mark.parametrize("shuffle", ["cpu", "device"])
def test_update_equals_the_hand_loop(shuffle, weight_sync, arithmetic):
    """a bc_coef schedule at progress 0.25 and a target_kl that never stops: the gated entry with the control block"""
    import torch

    import marl_sortingenv_amd as M
    from marl_sortingenv_amd.learner import PPO_BC_STAT_NAMES

    kw = dict(shuffle=shuffle, weight_sync=weight_sync, target_kl=1e9, clip_range_vf=K.C_VF)
    pol, flat, col, learner = _setup(arithmetic, bc_coef=lambda p: 2.0 * p, **kw)
    _, _, _, hand = _setup(arithmetic, bc_coef=0.5, **kw)
    data = {k: v.clone() for k, v in col.collect().items()}
    assert data["expert_actions"].shape == (K_STEPS, N_ENVS) and data["expert_actions"].dtype == torch.int32
    out = learner.update({k: v.clone() for k, v in data.items()}, progress_remaining=0.25)
    assert learner.bc_coef == 0.5 and out["stats"].shape == (EPOCHS * (TOTAL // BS), 12)
    M.compute_gae(data, hand.gamma, hand.gae_lambda)
    n_mb = EPOCHS * (TOTAL // BS)
    stats = torch.zeros((n_mb, 12), device="cuda")
    control = torch.zeros(2, dtype=torch.int32, device="cuda")
    i = 0
    for e in range(EPOCHS):
        perm = learner.last_permutations[e] if shuffle == "cpu" else hand.permutation(TOTAL, e)
        rows = perm.cuda()
        for start in range(0, TOTAL, BS):
            mb = rows[start:start + BS]
            hand.loss_grad(data, mb, mb.numel(), stats[i], control=control, target_kl=1e9)
            hand.adam_step(control)
            i += 1
    torch.cuda.synchronize()
    assert i == n_mb == 8 and learner.step == n_mb and control.tolist() == [0, n_mb]
    for name in ("weights", "m", "v"):
        assert same_bits(getattr(learner, name), getattr(hand, name)), name
    assert same_bits(out["stats"], stats) and not out["stopped"] and out["minibatches_run"] == n_mb
    assert np.array_equal(pol.flat_weights().view(np.uint32), learner.weights.cpu().numpy().view(np.uint32))
    assert set(out["mean"]) == set(PPO_BC_STAT_NAMES[:11])
    mean = stats.mean(dim=0).cpu()
    for j, name in enumerate(PPO_BC_STAT_NAMES[:11]):
        assert out["mean"][name] == pytest.approx(float(mean[j]), rel=1e-6, abs=1e-9), name
    assert 0.0 < out["mean"]["bc_loss"] and 0.0 <= out["mean"]["bc_unusable"] < 0.5 and 0.0 <= out["mean"]["bc_accuracy"] <= 1.0


def test_without_bc_coef_the_learner_is_what_it_was():
    import torch

    import marl_sortingenv_amd as M

    pol, flat, col, learner = _setup()
    assert learner.bc_coef is None and learner.workspace.numel() == learner.L.mse_ppo_workspace_bytes(*MONO)
    hp, sd = learner.hyperparameters(), learner.state_dict()
    assert "bc_coef" not in hp and "bc_coef" not in sd and hp["scheduled"] == []
    out = learner.update(col.collect())  # labels in the data are ignored
    assert out["stats"].shape[1] == 8 and set(out["mean"]) == set(R.STAT_NAMES)
    rec = learner.learn(col, 1)[0]
    assert "bc_coef" not in rec and "bc_loss" not in rec
    with_bc = _setup(bc_coef=0.5)[3]
    assert with_bc.hyperparameters() == dict(hp, bc_coef=0.5) and with_bc.state_dict()["bc_coef"] == 0.5
    rec = with_bc.learn(_setup()[2], 1)[0]
    assert rec["bc_coef"] == 0.5 and rec["bc_loss"] > 0.0 and "bc_accuracy" in rec and "bc_unusable" in rec
    scheduled = _setup(bc_coef=lambda p: p)[3]
    assert scheduled.hyperparameters() == dict(hp, scheduled=["bc_coef"])
    assert torch.cuda.is_available()
