"""GPU: SB3's clip_range_vf in both gradient kernels (mse_ppo_loss_grad_vclip -> the VCLIP instantiations of k_ppo_grad and
k_ppo_grad_matrix), the learner's schedules and the explained variance (mse_explained_variance).

The clipped gradient is held against the float64 autograd of tests/ppo_vclip_reference.py under the tolerance rule of
tests/ppo_reference.py (4 x torch's own float32 error, computed each run) on rows that keep the clamp's indicator away
from its discontinuity; every test asserts the margins on the float64 reference before it uses the rows."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import ppo_reference as R
from tests import ppo_vclip_reference as V
from tests.ppo_checks import DIM_MATRIX, HP, ROWS_PER_GROUP, bits, cpu_rows, device_rows, group_cap, make_learner, make_policy, same_bits
from tests.test_ppo_vclip_cpu import EV_BOUND, EV_SIZES, ev_inputs, ev_numpy

pytestmark = pytest.mark.gpu

MONO = (29, 22)
FORMS = ["fma", "matrix"]
C_VF = V.GPU_C


def vclip_learner(D, A, seed, arithmetic, c=C_VF, normalize=True):
    learner, flat = make_learner(D, A, seed, normalize=normalize, arithmetic=arithmetic)
    learner.clip_range_vf = c
    return learner, flat


def vclip_rows(D, A, n, seed, flat, c=C_VF):
    """-> (the seven CPU tensors obs, mk, actions, old_logp, adv, ret, old_values; the device dict with "values")"""
    obs, mask, mk, actions, old_logp, adv, ret, old = V.make_vclip_rows(D, A, n, seed, flat, True, c)
    V.assert_margins(flat, D, A, obs, mk, ret, old, c)
    data = device_rows(obs, mk, actions, old_logp, adv, ret)
    data["values"] = old.contiguous().cuda()
    return [obs, mk, actions, old_logp, adv, ret, old], data


def reference(D, A, flat, cpu, rows, c=C_VF, normalize=True):
    """(g64, s64, g32, s32) of the clipped loss on cpu[rows]"""
    import torch

    sel = [t if rows is None else t[rows] for t in cpu]
    args = (D, A, *sel, HP["clip_range"], HP["ent_coef"], HP["vf_coef"], c, normalize)
    return (*V.loss_and_grad(flat, torch.float64, *args), *V.loss_and_grad(flat, torch.float32, *args))


def check_vclip(D, A, flat, learner, cpu, data, rows_cpu, label, batch=None, yardstick_rows=None, ref=None, grad_out=None,
                stats_out=None):
    """tests/ppo_checks.py's check_loss_grad for the clipped loss: one loss_grad on `rows_cpu` (None: rows 0 .. batch - 1,
    rows_dev = NULL), twice (bit-equal), against float64.  yardstick_rows (B <= 2): the bound takes the largest float32
    error among these row sets as well - torch alone.  ref: a reference computed before (shared between the forms)."""
    import torch

    total = cpu[0].shape[0]
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
    assert same_bits(g, g2) and same_bits(stats, stats2), "two calls with the same inputs must agree bit for bit"
    if ref is None:
        ref = reference(D, A, flat, cpu, rows_cpu if rows_cpu is not None else (None if batch == total else torch.arange(batch)),
                        normalize=bool(learner.params.normalize_advantage))
    g64, s64, g32, s32 = ref
    scale, allowed = R.grad_bound(g64, g32)
    e32_others = 0.0
    if yardstick_rows is not None:
        for r in yardstick_rows:
            o64, t64, o32, t32 = reference(D, A, flat, cpu, r.reshape(-1))
            allowed = max(allowed, R.grad_bound(o64, o32)[1])
            e32_others = max(e32_others, float((t32.double() - t64).abs().max()))
    err = float((g.cpu().double() - g64).abs().max()) / scale
    serr = np.abs(stats.cpu().double().numpy() - s64.numpy())
    print(f"{label}: kernel grad err {err:.3e}, f32 yardstick {allowed / 4:.3e} (allowed {allowed:.3e}); "
          f"stats err {serr.max():.3e}, f32 stats err {float((s32.double() - s64).abs().max()):.3e}; value_loss {float(s64[2]):.6f}")
    assert torch.isfinite(g).all() and torch.isfinite(stats).all(), label
    assert err <= allowed, (label, err, allowed)
    assert np.all(serr <= R.stats_bound(s64, s32, e32_others)), (label, stats.cpu(), s64)
    return g, stats


# ---- 1. both forms against float64 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arithmetic", FORMS)
@pytest.mark.parametrize("D,A", DIM_MATRIX)
def test_every_shape(arithmetic, D, A):
    learner, flat = vclip_learner(D, A, D * 100 + A, arithmetic)
    cpu, data = vclip_rows(D, A, 300, 11, flat)  # four full tiles and a 44-row tail
    check_vclip(D, A, flat, learner, cpu, data, None, f"{arithmetic} vclip {D}->{A} B=300")


@pytest.mark.parametrize("arithmetic", FORMS)
@pytest.mark.parametrize("B", V.EDGE_BATCHES)
@pytest.mark.parametrize("D,A", V.EDGE_SHAPES)
def test_tile_edges(arithmetic, D, A, B):
    import torch

    learner, flat = vclip_learner(D, A, 41, arithmetic)
    cpu, data = vclip_rows(D, A, V.EDGE_ROWS, B, flat)
    perm = torch.randperm(V.EDGE_ROWS, generator=torch.Generator().manual_seed(B))
    for rows, name in ((None, "rows_dev=NULL"), (perm[:B], "permuted rows_dev")):
        yard = None
        if B <= 2:  # tests/ppo_checks.py batch_edges: the largest float32 error over 64 evaluations on other rows
            others = torch.arange(B, B + 64 * B) if rows is None else perm[B:B + 64 * B]
            yard = others.reshape(64, B)
        check_vclip(D, A, flat, learner, cpu, data, rows, f"{arithmetic} vclip {D}->{A} B={B} {name}", batch=B, yardstick_rows=yard)


@pytest.fixture(scope="module")
def past_the_cap():
    """one row set and one reference for both forms: a workgroup makes a second pass, both tile slots of workgroup 0"""
    D, A = MONO
    flat = R.random_flat(D, A, V.CAP_FLAT_SEED)
    cpu, data = vclip_rows(D, A, ROWS_PER_GROUP * group_cap() + 65, V.CAP_ROW_SEED, flat)
    return flat, cpu, data, reference(D, A, flat, cpu, None)


@pytest.mark.parametrize("arithmetic", FORMS)
def test_a_second_pass_of_a_workgroup(past_the_cap, arithmetic):
    D, A = MONO
    flat, cpu, data, ref = past_the_cap
    learner, _ = vclip_learner(D, A, V.CAP_FLAT_SEED, arithmetic)
    check_vclip(D, A, flat, learner, cpu, data, None, f"{arithmetic} vclip mono B={cpu[0].shape[0]} (cap {group_cap()})", ref=ref)


# ---- 2. the entry point: off is the old path, clipping touches only the critic, the gate, nothing else is written --------------
@pytest.fixture(scope="module")
def small():
    D, A = MONO
    flat = R.random_flat(D, A, V.SMALL_FLAT_SEED)
    cpu, data = vclip_rows(D, A, 300, V.SMALL_ROW_SEED, flat)
    return flat, cpu, data


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _raw(learner, data, flat_dev, entry, tail, fill=0.0):
    """one raw call of `entry` on rows 0 .. 299 with `tail` behind mse_ppo_loss_grad's 17 arguments -> (grad, stats)"""
    import torch

    D, A = MONO
    g = torch.full((flat_dev.numel(),), fill, device="cuda")
    s = torch.full((8,), fill, device="cuda")
    args = (D, A, _ptr(flat_dev), 300, None, 300, _ptr(data["observations"]), _ptr(data["action_masks"]), _ptr(data["actions"]),
            _ptr(data["log_probs"]), _ptr(data["advantages"]), _ptr(data["returns"]), C.byref(learner.params), _ptr(g), _ptr(s),
            _ptr(learner.workspace), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert getattr(learner.L, entry)(*args, *tail) == 0, learner.L.mse_last_error()
    torch.cuda.synchronize()
    return g, s


@pytest.mark.parametrize("gated", [False, True])
@pytest.mark.parametrize("arithmetic", FORMS)
def test_without_old_values_it_is_the_existing_entry_point(small, arithmetic, gated):
    import torch

    flat, cpu, data = small
    learner, _ = make_learner(*MONO, V.SMALL_FLAT_SEED, arithmetic=arithmetic)
    w = flat.cuda()
    code = FORMS.index(arithmetic)
    controls = [torch.zeros(2, dtype=torch.int32, device="cuda") for _ in range(2)] if gated else [None, None]
    # clip_range_vf is not read without old_values: NaN passes
    got = _raw(learner, data, w, "mse_ppo_loss_grad_vclip", (0.01, _ptr(controls[0]), code, None, float("nan")))
    if arithmetic == "matrix":
        want = _raw(learner, data, w, "mse_ppo_loss_grad_matrix", (0.01, _ptr(controls[1])))
    elif gated:
        want = _raw(learner, data, w, "mse_ppo_loss_grad_gated", (0.01, _ptr(controls[1])))
    else:
        want = _raw(learner, data, w, "mse_ppo_loss_grad", ())
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    assert bool(torch.isfinite(got[0]).all()) and float(got[0].abs().max()) > 0.0
    if gated:
        assert controls[0].tolist() == controls[1].tolist() and controls[0][1].item() == 1
    # ... and the learner without clip_range_vf calls exactly that
    stats = torch.zeros(8, device="cuda")
    g = learner.loss_grad(data, None, 300, stats, weights=w, grad_out=torch.zeros_like(got[0]),
                          control=None if not gated else torch.zeros(2, dtype=torch.int32, device="cuda"), target_kl=0.01)
    torch.cuda.synchronize()
    assert same_bits(g, want[0]) and same_bits(stats, want[1])


@pytest.mark.parametrize("arithmetic", FORMS)
def test_clipping_touches_only_the_critic(small, arithmetic):
    flat, cpu, data = small
    learner, _ = make_learner(*MONO, V.SMALL_FLAT_SEED, arithmetic=arithmetic)
    w = flat.cuda()
    code = FORMS.index(arithmetic)
    off = _raw(learner, data, w, "mse_ppo_loss_grad_vclip", (0.0, None, code, None, 0.0))
    on = _raw(learner, data, w, "mse_ppo_loss_grad_vclip", (0.0, None, code, _ptr(data["values"]), C_VF))
    vf_w1 = 32 * MONO[0] + 32 + 32 * 32 + 32 + MONO[1] * 32 + MONO[1]  # flat_layout(D, A).vf_w1: where the critic starts
    assert vf_w1 == R.num_weights(*MONO) - (32 * MONO[0] + 32 + 32 * 32 + 32 + 32 + 1)
    assert same_bits(off[0][:vf_w1], on[0][:vf_w1])
    assert not same_bits(off[0][vf_w1:], on[0][vf_w1:])
    keep = [1, 3, 4, 5, 6, 7]
    assert same_bits(off[1][keep], on[1][keep])
    assert float(off[1][2]) != float(on[1][2]) and float(off[1][0]) != float(on[1][0])  # value_loss, and the loss with it


@pytest.mark.parametrize("arithmetic", FORMS)
def test_gate(small, arithmetic):
    import torch

    flat, cpu, data = small
    learner, _ = vclip_learner(*MONO, V.SMALL_FLAT_SEED, arithmetic)
    w = flat.cuda()
    code = FORMS.index(arithmetic)
    nan = float("nan")
    old = _ptr(data["values"])
    g0, s0 = _raw(learner, data, w, "mse_ppo_loss_grad_vclip", (0.0, None, code, old, C_VF), fill=nan)  # the ungated dry run
    kl = float(s0[4])
    assert kl > 0.0 and bool(torch.isfinite(g0).all()) and bool(torch.isfinite(s0).all())
    # closed on entry: neither output is written, the block is unchanged
    control = torch.tensor([1, 5], dtype=torch.int32, device="cuda")
    g, s = _raw(learner, data, w, "mse_ppo_loss_grad_vclip", (1e9, _ptr(control), code, old, C_VF), fill=nan)
    assert control.tolist() == [1, 5]
    assert bool(torch.isnan(g).all()) and bool(torch.isnan(s).all())
    # open, a threshold below this minibatch's approx_kl: counted, and the flag set
    control = torch.zeros(2, dtype=torch.int32, device="cuda")
    g, s = _raw(learner, data, w, "mse_ppo_loss_grad_vclip", (0.5 * kl / 1.5, _ptr(control), code, old, C_VF), fill=nan)
    assert control.tolist() == [1, 1] and same_bits(g, g0) and same_bits(s, s0)
    # open, a threshold above it: counted, not stopped; through the learner this time
    control = torch.zeros(2, dtype=torch.int32, device="cuda")
    s = torch.full((8,), nan, device="cuda")
    g = learner.loss_grad(data, None, 300, s, weights=w, grad_out=torch.full_like(g0, nan), control=control, target_kl=2.0 * kl / 1.5)
    torch.cuda.synchronize()
    assert control.tolist() == [0, 1] and same_bits(g, g0) and same_bits(s, s0)


@pytest.mark.parametrize("arithmetic", FORMS)
def test_writes_its_outputs_and_nothing_else(small, arithmetic):
    import torch

    D, A = MONO
    flat, cpu, data = small
    learner, _ = vclip_learner(D, A, V.SMALL_FLAT_SEED, arithmetic)
    W, band, sentinel = flat.numel(), 64, 12345.0
    gbuf = torch.full((W + 2 * band,), sentinel, device="cuda")
    sbuf = torch.full((8 + 2 * band,), sentinel, device="cuda")
    gbuf[band:band + W] = float("nan")
    sbuf[band:band + 8] = float("nan")
    check_vclip(D, A, flat, learner, cpu, data, None, f"{arithmetic} vclip into banded buffers", grad_out=gbuf[band:band + W],
                stats_out=sbuf[band:band + 8])
    for buf, n in ((gbuf, W), (sbuf, 8)):
        assert bool((buf[:band] == sentinel).all()) and bool((buf[band + n:] == sentinel).all())
        assert int(torch.isfinite(buf[band:band + n]).sum()) == n


# ---- 3. update() and learn() -------------------------------------------------------------------------------------------------------
N_ENVS, K_STEPS, EPOCHS, BS, SEED = 64, 8, 2, 128, 5
TOTAL = N_ENVS * K_STEPS
PLAIN_KEYS = set(R.STAT_NAMES) | {"reward"}


def _setup(arithmetic="fma", **kw):
    import marl_sortingenv_amd as M

    pol, flat = make_policy(*MONO, 31)
    env = M.BatchedSortingEnv(kind="mono", num_envs=N_ENVS, device=0, base_seed=21, max_steps=5, noise_sorting=0.05, balesize=200,
                              auto_reset=True)
    col = M.FusedPolicyRollout(env, pol, K_STEPS, seed=22)
    kw = {**HP, "learning_rate": 1e-3, **kw}
    learner = M.PPOLearner(pol, n_epochs=EPOCHS, batch_size=BS, seed=SEED, arithmetic=arithmetic, shuffle="device", **kw)
    return pol, flat, col, learner


def _same_learner(a, b, label):
    for name in ("weights", "m", "v"):
        assert same_bits(getattr(a, name), getattr(b, name)), (label, name)
    assert a.step == b.step, label


# c = 0.2 leaves the first update of a fresh rollout unclipped (the values have moved less than that from the rollout's by
# its last minibatch); 0.002 is passed after one Adam step of 1e-3 per weight, so there the clamp is at work inside update()
@pytest.mark.parametrize("c", [C_VF, 0.002])
@pytest.mark.parametrize("arithmetic", FORMS)
def test_update_with_clip_range_vf_equals_the_hand_loop(arithmetic, c):
    import torch

    import marl_sortingenv_amd as M

    pol, flat, col, learner = _setup(arithmetic, clip_range_vf=c)
    _, _, _, hand = _setup(arithmetic, clip_range_vf=c)
    data = {k: v.clone() for k, v in col.collect().items()}
    assert data["values"].shape == (K_STEPS, N_ENVS) and data["values"].dtype == torch.float32 and data["values"].is_contiguous()
    out = learner.update({k: v.clone() for k, v in data.items()})
    # by hand: permutation(), loss_grad() and adam_step()
    M.compute_gae(data, hand.gamma, hand.gae_lambda)
    n_mb = EPOCHS * (TOTAL // BS)
    stats = torch.zeros((n_mb, 8), device="cuda")
    first_rows = first_grad = None
    i = 0
    for e in range(EPOCHS):
        perm = hand.permutation(TOTAL, e)
        rows = perm.cuda()
        for start in range(0, TOTAL, BS):
            mb = rows[start:start + BS]
            g = hand.loss_grad(data, mb, mb.numel(), stats[i])
            if i == 0:
                first_rows, first_grad = perm[:BS], g.clone()
            hand.adam_step()
            i += 1
    torch.cuda.synchronize()
    assert i == n_mb == 8 and learner.step == n_mb and learner.last_epochs == [0, 1]
    _same_learner(learner, hand, "update with clip_range_vf")
    assert same_bits(out["stats"], stats)
    assert np.array_equal(pol.flat_weights().view(np.uint32), learner.weights.cpu().numpy().view(np.uint32))
    # the first minibatch's gradient (the initial weights) against float64 on the rollout's own values
    cpu = cpu_rows(data, first_rows) + [data["values"].reshape(-1).cpu()[first_rows]]
    g64, s64, g32, s32 = reference(*MONO, flat, cpu, None, c=c)
    scale, allowed = R.grad_bound(g64, g32)
    err = float((first_grad.cpu().double() - g64).abs().max()) / scale
    with torch.no_grad():
        d = R.forward(flat.double(), *MONO, cpu[0].double(), cpu[1])[1] - cpu[6].double()
    print(f"{arithmetic} c={c} first minibatch of update(): grad err {err:.3e} (allowed {allowed:.3e}); {int((d.abs() > c).sum())} of {BS} "
          f"rows clipped, the nearest {float((d.abs() - c).abs().min()):.3e} from the edge")
    assert err <= allowed
    assert np.all(np.abs(out["stats"][0].cpu().double().numpy() - s64.numpy()) <= R.stats_bound(s64, s32))
    allrows = cpu_rows(data)
    with torch.no_grad():
        d_end = R.forward(learner.weights.cpu().double(), *MONO, allrows[0].double(), allrows[1])[1] - data["values"].reshape(-1).cpu().double()
    moved = float((d_end.abs() > c).double().mean())
    print(f"{arithmetic} c={c}: after the update {moved:.2f} of the rows have |value - old| > c (largest {float(d_end.abs().max()):.3e})")
    if c != C_VF:  # the clamp was at work: the range decides what the update leaves
        assert moved > 0.1
        _, _, _, wide = _setup(arithmetic, clip_range_vf=C_VF)
        wide.update({k: v.clone() for k, v in data.items()})
        assert not same_bits(wide.weights, learner.weights)


def test_schedules_in_learn_equal_updates_with_the_constants_set_by_hand():
    import torch

    lr, clip = (lambda p: 3e-4 * p), (lambda p: 0.1 + 0.1 * p)
    pol, _, col, learner = _setup(learning_rate=lr, clip_range=clip)
    pol_b, _, col_b, hand = _setup(learning_rate=0.123, clip_range=0.3)
    assert learner.progress_remaining == 1.0 and learner.learning_rate == 3e-4 and learner.clip_range == 0.2
    history = learner.learn(col, 3)
    ps = [1.0 - (it + 1) / 3 for it in range(3)]
    assert ps[2] == 0.0 and learner.progress_remaining == 0.0
    for p in ps:
        hand.learning_rate = 3e-4 * p
        hand.params.clip_range = 0.1 + 0.1 * p
        hand.update(col_b.collect())
    torch.cuda.synchronize()
    _same_learner(learner, hand, "learn with schedules")
    assert np.array_equal(pol.flat_weights().view(np.uint32), pol_b.flat_weights().view(np.uint32))
    for rec, p in zip(history, ps):
        assert set(rec) == PLAIN_KEYS | {"learning_rate", "clip_range"}
        assert rec["learning_rate"] == 3e-4 * p and rec["clip_range"] == 0.1 + 0.1 * p
    # the last update ran with a learning rate of 0: it changed no weight
    w2 = hand.weights.clone()
    hand.learning_rate = 0.0
    hand.update(col_b.collect())
    assert same_bits(hand.weights, w2)
    # update(progress_remaining=...) sets the progress and evaluates the schedules once
    calls = []
    _, _, col_c, third = _setup(learning_rate=lambda p: calls.append(p) or 1e-3 * (1 + p), clip_range_vf=lambda p: 0.1 + p)
    calls.clear()
    third.update(col_c.collect(), progress_remaining=0.25)
    assert calls == [0.25] and third.progress_remaining == 0.25
    assert third.learning_rate == 1e-3 * 1.25 and third.clip_range_vf == 0.1 + 0.25 and third.clip_range == 0.2


def test_plain_floats_leave_the_records_as_they_were():
    _, _, col, learner = _setup()
    history = learner.learn(col, 2)
    assert [set(rec) for rec in history] == [PLAIN_KEYS] * 2
    _, _, col, learner = _setup(clip_range_vf=C_VF)
    history = learner.learn(col, 1, explained_variance=True)
    assert set(history[0]) == PLAIN_KEYS | {"clip_range_vf", "explained_variance"} and history[0]["clip_range_vf"] == C_VF


# ---- 4. the explained variance -----------------------------------------------------------------------------------------------------
def _ev_device(L, values, returns, workspace=None):
    """-> (the f32 the device wrote, as numpy; the banded buffer around it)"""
    import torch

    n = values.size
    v, r = torch.from_numpy(values).cuda(), torch.from_numpy(returns).cuda()
    out = torch.full((129,), 12345.0, device="cuda")
    if workspace is None:
        workspace = torch.empty(int(L.mse_explained_variance_workspace_bytes()), dtype=torch.uint8, device="cuda")
    status = L.mse_explained_variance(n, _ptr(v), _ptr(r), _ptr(out[64:]), _ptr(workspace), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert status == 0, L.mse_last_error()
    host = out.cpu().numpy()
    assert np.all(host[:64] == 12345.0) and np.all(host[65:] == 12345.0)  # writes only out_dev[0]
    assert bool(torch.equal(v.cpu(), torch.from_numpy(values))) and bool(torch.equal(r.cpu(), torch.from_numpy(returns)))
    return host[64]


def _ev_host(L, values, returns):
    out = np.zeros(1, np.float32)
    assert L.mse_explained_variance_host(values.size, values.ctypes.data_as(C.c_void_p), returns.ctypes.data_as(C.c_void_p),
                                         out.ctypes.data_as(C.c_void_p)) == 0
    return out[0]


@pytest.mark.parametrize("n", EV_SIZES)
def test_explained_variance_equals_its_host_twin(n):
    import marl_sortingenv_amd as M

    L = M.load_library()
    values, returns = ev_inputs(n)
    got, host, want = _ev_device(L, values, returns), _ev_host(L, values, returns), ev_numpy(values, returns)
    print(f"n={n}: device {got!r}, host {host!r}, numpy float64 {want!r}")
    assert got.tobytes() == host.tobytes()
    assert _ev_device(L, values, returns).tobytes() == got.tobytes()
    if n == 1:
        assert math.isnan(got)
        return
    assert abs(float(got) - want) <= EV_BOUND * max(1.0, abs(want))
    assert _ev_device(L, returns, returns) == 1.0
    assert math.isnan(_ev_device(L, values, np.full(n, 10.25, np.float32)))
    worse = (-3 * values).astype(np.float32)
    assert _ev_device(L, worse, returns).tobytes() == _ev_host(L, worse, returns).tobytes()


@pytest.mark.parametrize("target_kl", [None, 1e9])
def test_update_reports_the_explained_variance(target_kl):
    import marl_sortingenv_amd as M

    _, _, col, learner = _setup(target_kl=target_kl)
    _, _, _, plain = _setup(target_kl=target_kl)
    data = {k: v.clone() for k, v in col.collect().items()}
    out = learner.update(data, explained_variance=True)
    want = _ev_host(learner.L, data["values"].reshape(-1).cpu().numpy(), data["returns"].reshape(-1).cpu().numpy())
    print(f"explained variance of the rollout: {out['explained_variance']!r}")
    assert out["explained_variance"] == float(want) and math.isfinite(out["explained_variance"])
    # asking for it changes nothing else
    ref = plain.update({k: v.clone() for k, v in data.items() if k not in ("advantages", "returns")})
    assert "explained_variance" not in ref and set(out) == set(ref) | {"explained_variance"}
    _same_learner(learner, plain, "update(explained_variance=True)")
    assert same_bits(out["stats"], ref["stats"]) and out["mean"] == ref["mean"]
    # the learner's workspace serves: the same bits as with one of the kernel's own size
    assert _ev_device(M.load_library(), data["values"].reshape(-1).cpu().numpy(), data["returns"].reshape(-1).cpu().numpy(),
                      workspace=learner.workspace).tobytes() == want.tobytes()
