"""CPU checks of value clipping (SB3's clip_range_vf), the schedule helper and the explained variance (no device needed).

marl-sortingenv_amd/csrc/mse_ppo_math.h is compiled on the host through a shim of this file's own, which composes the
header's per-row pieces as the gradient kernels do with value_head_terms_clipped in the critic, and is held against the
float64 autograd of tests/ppo_vclip_reference.py under the tolerance rule of tests/ppo_reference.py (4 x the error of
torch's own float32 evaluation, computed each run).  The rows keep the clamp's indicator away from its discontinuity
(tests/ppo_vclip_reference.py says how); every test asserts that on the float64 reference before it uses them."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import marl_sortingenv_amd as M
from marl_sortingenv_amd._lib import EXPORTS, MsePpoParams
from tests import ppo_reference as R
from tests import ppo_vclip_reference as V
from tests.ppo_checks import DIM_MATRIX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "marl-sortingenv_amd", "csrc")
INVALID, ALIGNMENT, NO_DEVICE = -1, -6, -3

SHIM = r"""
#include "mse_ppo_math.h"
#include <vector>
using namespace mseppo;

template <int N>
static void outer(float *gw, float *gb, const float *d, int n_out, const float *a, int ld)
{
    for (int o = 0; o < n_out; ++o) {
        for (int i = 0; i < N; ++i) gw[o * ld + i] = fmaf(d[o], a[i], gw[o * ld + i]);
        gb[o] += d[o];
    }
}

// a minibatch as k_ppo_grad<DP, AP, true> composes it: the actor as ever, the critic through value_head_terms_clipped
template <int DP, int AP>
static void run(int D, int A, const float *wflat, long B, const float *obs, const unsigned char *mask, const int *act,
                const float *old_logp, const float *adv, const float *ret, const float *old_values, Params P, float *grad,
                double *stats)
{
    typedef Padded<DP, AP> PW;
    const Flat F = flat_layout(D, A);
    std::vector<float> w(PW::total, 0.0f), g(PW::total, 0.0f);
    for (int f = 0; f < F.total; ++f) w[padded_index<DP, AP>(f, D, A)] = wflat[f];
    float mean = 0.0f, std = 1.0f;
    const bool normalize = P.normalize_advantage != 0 && B > 1;
    if (normalize) {
        double s = 0.0, q = 0.0;
        for (long b = 0; b < B; ++b) s += adv[b];
        for (long b = 0; b < B; ++b) q += (adv[b] - s / B) * (adv[b] - s / B);
        mean = (float)(s / B);
        std = (float)sqrt(q / (B - 1));
    }
    const float inv_b = 1.0f / (float)B;
    double sums[5] = {0, 0, 0, 0, 0};
    for (long b = 0; b < B; ++b) {
        float x[DP];
        for (int i = 0; i < DP; ++i) x[i] = i < D ? obs[b * D + i] : 0.0f;
        unsigned legal = 0;
        for (int a = 0; a < A; ++a) legal |= (mask == nullptr || mask[b * A + a] ? 1u : 0u) << a;
        const float a_used = normalize ? normalized_advantage(adv[b], mean, std) : adv[b];
        float h1[kH], h2[kH], dz2[kH], dz1[kH], dl[AP];
        hidden_forward<DP>(&w[PW::pi_w1], &w[PW::pi_b1], &w[PW::pi_w2], &w[PW::pi_b2], x, h1, h2);
        head_forward<AP>(&w[PW::act_w], &w[PW::act_b], h2, dl);
        const PolicyTerms t = policy_head_terms<AP>(dl, A, legal, act[b], old_logp[b], a_used, P, inv_b);
        sums[0] += t.surrogate; sums[2] += t.entropy; sums[3] += t.kl; sums[4] += t.clipped;
        outer<kH>(&g[PW::act_w], &g[PW::act_b], dl, AP, h2, kH);
        backprop<AP>(&w[PW::act_w], dl, h2, dz2);
        outer<kH>(&g[PW::pi_w2], &g[PW::pi_b2], dz2, kH, h1, kH);
        backprop<kH>(&w[PW::pi_w2], dz2, h1, dz1);
        outer<DP>(&g[PW::pi_w1], &g[PW::pi_b1], dz1, kH, x, DP);
        hidden_forward<DP>(&w[PW::vf_w1], &w[PW::vf_b1], &w[PW::vf_w2], &w[PW::vf_b2], x, h1, h2);
        float v[1], dv[1];
        head_forward<1>(&w[PW::val_w], &w[PW::val_b], h2, v);
        sums[1] += value_head_terms_clipped(v[0], old_values[b], ret[b], P, inv_b, dv[0]);
        outer<kH>(&g[PW::val_w], &g[PW::val_b], dv, 1, h2, kH);
        backprop<1>(&w[PW::val_w], dv, h2, dz2);
        outer<kH>(&g[PW::vf_w2], &g[PW::vf_b2], dz2, kH, h1, kH);
        backprop<kH>(&w[PW::vf_w2], dz2, h1, dz1);
        outer<DP>(&g[PW::vf_w1], &g[PW::vf_b1], dz1, kH, x, DP);
    }
    for (int f = 0; f < F.total; ++f) grad[f] = g[padded_index<DP, AP>(f, D, A)];
    const double pl = sums[0] / B, vl = sums[1] / B, el = -sums[2] / B;
    stats[0] = pl + P.ent_coef * el + P.vf_coef * vl; stats[1] = pl; stats[2] = vl; stats[3] = el;
    stats[4] = sums[3] / B; stats[5] = sums[4] / B; stats[6] = mean; stats[7] = std;
}

extern "C" {
int ppo_rows_vclip(int D, int A, const float *wflat, long B, const float *obs, const unsigned char *mask, const int *act,
                   const float *old_logp, const float *adv, const float *ret, const float *old_values, float clip, float ent,
                   float vf, int norm, float clip_vf, float *grad, double *stats)
{
    Params P{clip, ent, vf, norm, clip_vf};
    const GradShape shape = select_grad_shape(D, A);
    if (shape == kShapeNone) return -1;
#define SHIM_RUN(DP, AP) run<DP, AP>(D, A, wflat, B, obs, mask, act, old_logp, adv, ret, old_values, P, grad, stats)
    MSE_PPO_DISPATCH(shape, SHIM_RUN);
#undef SHIM_RUN
    return 0;
}
// Params as every caller from before the trailing member builds it: clip_range_vf is 0
float four_member_params_clip_vf(void) { Params P{0.2f, 0.05f, 0.5f, 1}; return P.clip_range_vf; }
float value_terms(float value, float ret, float vf, float inv_b, float *dv)
{
    Params P{0.2f, 0.0f, vf, 1};
    return value_head_terms(value, ret, P, inv_b, *dv);
}
float value_terms_clipped(float value, float old_value, float ret, float vf, float c, float inv_b, float *dv)
{
    Params P{0.2f, 0.0f, vf, 1, c};
    return value_head_terms_clipped(value, old_value, ret, P, inv_b, *dv);
}
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler to build the mse_ppo_math.h shim")
    d = tmp_path_factory.mktemp("ppo_vclip")
    src, so = d / "shim.cpp", d / "shim.so"
    src.write_text(SHIM)
    subprocess.run([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-I", CSRC,
                    str(src), "-o", str(so)], check=True)
    L = C.CDLL(str(so))
    L.four_member_params_clip_vf.restype = C.c_float
    L.value_terms.restype = C.c_float
    L.value_terms.argtypes = [C.c_float] * 4 + [C.POINTER(C.c_float)]
    L.value_terms_clipped.restype = C.c_float
    L.value_terms_clipped.argtypes = [C.c_float] * 6 + [C.POINTER(C.c_float)]
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


HP = dict(clip_range=0.2, ent_coef=0.05, vf_coef=0.5)


def run_shim(shim, D, A, flat, obs, mk, actions, old_logp, adv, ret, old, c, normalize):
    B = obs.shape[0]
    grad = np.zeros(R.num_weights(D, A), np.float32)
    stats = np.zeros(8, np.float64)
    m8 = None if mk is None else np.ascontiguousarray(mk.numpy().astype(np.uint8))
    rc = shim.ppo_rows_vclip(D, A, _p(flat.numpy()), C.c_long(B), _p(np.ascontiguousarray(obs.numpy())), _p(m8), _p(actions.numpy()),
                             _p(old_logp.numpy()), _p(adv.numpy()), _p(ret.numpy()), _p(old.numpy()), C.c_float(HP["clip_range"]),
                             C.c_float(HP["ent_coef"]), C.c_float(HP["vf_coef"]), int(normalize), C.c_float(c), _p(grad), _p(stats))
    assert rc == 0
    return torch.from_numpy(grad), torch.from_numpy(stats)


CASES = [(D, A, 300) for D, A in DIM_MATRIX] + [(29, 22, B) for B in (1, 2, 64, 65)]


@pytest.mark.parametrize("c", [0.05, 0.2])
@pytest.mark.parametrize("D,A,B", CASES)
def test_generated_rows_keep_their_margins(D, A, B, c):
    """every seed and shape the CPU and the GPU suite use (tests/test_gpu_ppo_vclip.py draws with the seeds below too)"""
    flat = R.random_flat(D, A, seed=D * 100 + A)
    for seed in (7 + B, 11, 1007 + B):
        n = 64 * B if seed == 1007 + B else B
        obs, mask, mk, actions, old_logp, adv, ret, old = V.make_vclip_rows(D, A, n, seed, flat, True, c)
        clipped = V.assert_margins(flat, D, A, obs, mk, ret, old, c)
        assert ret.dtype == old.dtype == torch.float32 and old.shape == ret.shape == (n,)
        if n >= 300:
            assert 0.3 * n < clipped < 0.7 * n  # about half


@pytest.mark.parametrize("cap", [512, 208])  # 2 x CUs capped at 512 on an MI355X; a smaller device's cap as well
def test_rows_of_the_gpu_suite_keep_their_margins(cap):
    for D, A, flat_seed, n, seed in V.gpu_row_sets(cap):
        flat = R.random_flat(D, A, flat_seed)
        obs, mask, mk, actions, old_logp, adv, ret, old = V.make_vclip_rows(D, A, n, seed, flat, True, V.GPU_C)
        clipped = V.assert_margins(flat, D, A, obs, mk, ret, old, V.GPU_C)
        assert 0.3 * n < clipped < 0.7 * n, (D, A, n, seed, clipped)


@pytest.mark.parametrize("c", [0.05, 0.2])
@pytest.mark.parametrize("D,A,B", CASES)
def test_header_clipped_loss_and_gradient_match_float64_autograd(shim, D, A, B, c):
    flat = R.random_flat(D, A, seed=D * 100 + A)
    obs, mask, mk, actions, old_logp, adv, ret, old = V.make_vclip_rows(D, A, B, 7 + B, flat, True, c)
    V.assert_margins(flat, D, A, obs, mk, ret, old, c)
    # B <= 2: the float32 yardstick is one draw of a heavy-tailed error, so the bound is the largest
    # float32 error over 64 evaluations of the same size on other rows - torch alone (tests/test_ppo_math_cpu.py)
    other = None
    if B <= 2:
        other = V.make_vclip_rows(D, A, 64 * B, 1007 + B, flat, True, c)
        V.assert_margins(flat, D, A, other[0], other[2], other[6], other[7], c)
    for normalize in (1, 0):
        tail = (HP["clip_range"], HP["ent_coef"], HP["vf_coef"], c, bool(normalize))
        args = (D, A, obs, mk, actions, old_logp, adv, ret, old, *tail)
        g64, s64 = V.loss_and_grad(flat, torch.float64, *args)
        g32, s32 = V.loss_and_grad(flat, torch.float32, *args)
        g, s = run_shim(shim, D, A, flat, obs, mk, actions, old_logp, adv, ret, old, c, normalize)
        scale, allowed = R.grad_bound(g64, g32)
        e32_others = 0.0
        if other is not None:
            for j in range(64):
                o = [t[j * B:(j + 1) * B] for t in (other[0], other[2], *other[3:])]
                a1 = (D, A, *o, *tail)
                (o64, t64), (o32, t32) = V.loss_and_grad(flat, torch.float64, *a1), V.loss_and_grad(flat, torch.float32, *a1)
                allowed = max(allowed, R.grad_bound(o64, o32)[1])
                e32_others = max(e32_others, float((t32.double() - t64).abs().max()))
        err = float((g.double() - g64).abs().max()) / scale
        print(f"D={D} A={A} B={B} c={c} normalize={normalize}: header grad err {err:.3e}, f32 yardstick {allowed / 4:.3e} "
              f"(allowed {allowed:.3e}); value_loss {float(s64[2]):.6f}")
        assert err <= allowed
        assert np.all(np.abs((s - s64).numpy()) <= R.stats_bound(s64, s32, e32_others)), (s, s64, e32_others)
        if B >= 300:  # clipping is at work: the unclipped loss differs, and so does the critic's gradient
            gu, su = R.loss_and_grad(flat, torch.float64, D, A, obs, mk, actions, old_logp, adv, ret, *tail[:3], bool(normalize))
            assert abs(float(su[2] - s64[2])) > 1e-3
            vf_w1 = R.num_weights(D, A) - (32 * D + 32 + 32 * 32 + 32 + 32 + 1)
            assert torch.equal(gu[:vf_w1], g64[:vf_w1]) and not torch.equal(gu[vf_w1:], g64[vf_w1:])


def _f32(x):
    return np.float32(x)


def test_header_value_terms(shim):
    """value_head_terms is what it was (numpy float32, every operation rounded separately, bit for bit); the clipped form
    is the issue's five operations, equals it inside the range and has no gradient outside"""
    assert shim.four_member_params_clip_vf() == 0.0
    rng = np.random.default_rng(5)
    dv = C.c_float(0.0)
    for value, ret, old in rng.standard_normal((200, 3)).astype(np.float32) * 2:
        for vf, inv_b in ((0.5, 1.0 / 300), (1.0, 1.0), (0.25, 1.0 / 7)):
            vf, inv_b = _f32(vf), _f32(inv_b)
            sq = shim.value_terms(value, ret, vf, inv_b, C.byref(dv))
            e = _f32(value - ret)
            assert _f32(sq) == _f32(e * e) and _f32(dv.value) == _f32(_f32(_f32(vf * _f32(2.0)) * e) * inv_b)
            for c in (_f32(0.05), _f32(0.2), _f32(10.0)):
                sqc = shim.value_terms_clipped(value, old, ret, vf, c, inv_b, C.byref(dv))
                d = _f32(value - old)
                dc = np.minimum(np.maximum(d, -c), c)
                ec = _f32(_f32(old + dc) - ret)
                assert _f32(sqc) == _f32(ec * ec)
                want = _f32(_f32(_f32(vf * _f32(2.0)) * ec) * inv_b) if d == dc else _f32(0.0)
                assert _f32(dv.value) == want
    # the closed range: exactly at +-c the clamp passes the gradient
    for d in (0.25, -0.25):
        shim.value_terms_clipped(1.0 + d, 1.0, 3.0, 0.5, 0.25, 1.0, C.byref(dv))
        assert dv.value == 0.5 * 2.0 * (1.0 + d - 3.0)
    shim.value_terms_clipped(1.5, 1.0, 3.0, 0.5, 0.25, 1.0, C.byref(dv))
    assert dv.value == 0.0


def test_vclip_entry_point_checks_its_arguments_before_any_device_call():
    L = M.load_library()
    for name in ("mse_ppo_loss_grad_vclip", "mse_explained_variance_workspace_bytes", "mse_explained_variance",
                 "mse_explained_variance_host"):
        assert hasattr(L, name) and name in EXPORTS
    assert L.mse_version() == 200
    one = C.c_void_p(16)  # a non-null pointer that is never followed: the calls below fail their argument checks
    p = MsePpoParams(C.sizeof(MsePpoParams), 0.2, 0.0, 0.5, 1)
    ok = [29, 22, one, 64, None, 64, one, None, one, one, one, one, C.byref(p), one, one, one, None, 0.01, None, 0, one, 0.2]

    def call(**change):
        a = list(ok)
        for k, v in change.items():
            a[int(k[1:])] = v
        return L.mse_ppo_loss_grad_vclip(*a)

    def refused(why, **change):
        L.mse_ppo_loss_grad(*([0] + ok[1:17]))  # leaves another message behind
        assert call(**change) == INVALID, change
        err = L.mse_last_error()
        assert b"mse_ppo_loss_grad_vclip" in err and why in err, (change, err)

    # the new checks
    for c in (0.0, -0.1, float("nan"), float("inf"), float("-inf"), 1e-60):
        for arithmetic in (0, 1):
            refused(b"clip_range_vf", a21=c, a19=arithmetic)
    for arithmetic in (-1, 2):
        refused(b"arithmetic", a19=arithmetic)
        refused(b"arithmetic", a19=arithmetic, a20=None)
    # the existing ones, through this entry point
    for i in (2, 6, 8, 9, 10, 11, 12, 13, 14, 15):
        refused(b"null", **{f"a{i}": None})
    for D, A in ((0, 22), (33, 22), (29, 0), (29, 33), (-1, 1)):
        refused(b"1..32", a0=D, a1=A)
    for size in (0, 3, C.sizeof(MsePpoParams) - 4, C.sizeof(MsePpoParams) + 4):
        bad = MsePpoParams(size, 0.2, 0.0, 0.5, 1)
        refused(b"struct_size", a12=C.byref(bad))
    refused(b"batch", a5=65)  # batch > n_rows without rows_dev
    refused(b"batch", a3=0)
    refused(b"batch", a5=0)
    nan = MsePpoParams(C.sizeof(MsePpoParams), float("nan"), 0.0, 0.5, 1)
    refused(b"clip_range /", a12=C.byref(nan))
    for off in (8, 4, 1):
        assert call(a15=C.c_void_p(16 + off)) == ALIGNMENT and b"16-byte aligned" in L.mse_last_error()
    refused(b"target_kl", a17=float("nan"), a18=one)
    # the documented order: target_kl, the existing checks in their order, the arithmetic, the clipping range
    bad = MsePpoParams(3, float("nan"), 0.0, 0.5, 1)
    refused(b"target_kl", a17=float("nan"), a18=one, a2=None)
    refused(b"null", a2=None, a0=0)
    refused(b"1..32", a0=0, a12=C.byref(bad))
    refused(b"struct_size", a12=C.byref(bad), a5=65)
    refused(b"batch", a5=65, a12=C.byref(nan))
    refused(b"clip_range /", a12=C.byref(nan), a15=C.c_void_p(24))
    assert call(a15=C.c_void_p(24), a19=2) == ALIGNMENT
    refused(b"arithmetic", a19=2, a21=0.0)
    if torch.cuda.is_available():
        return  # with a device the well-formed call would follow the pointers
    # well-formed: there is no device.  Without old_values clip_range_vf is not read, without a control block target_kl is not
    for arithmetic in (0, 1):
        assert call(a19=arithmetic) == NO_DEVICE and b"no HIP device" in L.mse_last_error()
        assert call(a19=arithmetic, a20=None, a21=float("nan")) == NO_DEVICE
        assert call(a19=arithmetic, a17=float("nan")) == NO_DEVICE
        assert call(a19=arithmetic, a18=one) == NO_DEVICE


def test_schedule_helper():
    from marl_sortingenv_amd.learner import resolve_schedule

    assert M.resolve_schedule is resolve_schedule
    for v in (3e-4, 0.2, 1, 7.5):
        for p in (1.0, 0.5, 0.0):
            got = resolve_schedule(v, p)
            assert got == float(v) and type(got) is float
    seen = []

    def linear(p):
        seen.append(p)
        return 3e-4 * p

    assert resolve_schedule(linear, 2 / 3) == 3e-4 * (2 / 3) and seen == [2 / 3]
    assert resolve_schedule(lambda p: np.float32(0.1) + np.float32(0.1) * np.float32(p), 0.5) == float(np.float32(0.1) + np.float32(0.05))
    for bad in (float("nan"), float("inf"), float("-inf"), -1e-9, 0.0, -0.0):
        with pytest.raises(ValueError, match="clip_range_vf"):
            resolve_schedule(bad, 1.0, "clip_range_vf")
        with pytest.raises(ValueError, match="learning_rate"):
            resolve_schedule(lambda p, bad=bad: bad, 0.25, "learning_rate")
    # a linear decay reaches 0 in its last update: admitted where the caller says so, and only 0
    assert resolve_schedule(linear, 0.0, "learning_rate", allow_zero=True) == 0.0
    for bad in (float("nan"), float("inf"), -1e-9):
        with pytest.raises(ValueError, match="learning_rate"):
            resolve_schedule(lambda p, bad=bad: bad, 0.0, "learning_rate", allow_zero=True)


def test_learner_takes_schedules_without_a_device():
    class _Policy:  # refused before anything of the policy is read
        pass

    for kw in (dict(clip_range_vf=0.0), dict(clip_range_vf=-0.2), dict(clip_range_vf=float("nan")), dict(clip_range_vf=lambda p: 0.0),
               dict(learning_rate=lambda p: -1.0), dict(clip_range=lambda p: float("inf"))):
        with pytest.raises(ValueError, match="|".join(kw)):
            M.PPOLearner(_Policy(), **kw)


def ev_numpy(values, returns):
    """SB3's explained_variance in float64 on the float32 inputs"""
    y, yp = returns.astype(np.float64), values.astype(np.float64)
    var_y = np.var(y)
    return np.nan if var_y == 0 else 1.0 - np.var(y - yp) / var_y


EV_SIZES = [1, 2, 255, 256, 257, 65537]
EV_BOUND = 2.0 ** -22  # the double sums leave about 1e-13, the one rounding to f32 half an ulp (2^-24 relative); doubled


def ev_inputs(n, seed=3):
    rng = np.random.default_rng(seed + n)
    returns = (10.0 + rng.standard_normal(n)).astype(np.float32)  # a mean offset of 10, unit spread
    values = (returns + 0.5 * rng.standard_normal(n)).astype(np.float32)
    return values, returns


def ev_host(L, values, returns):
    out = np.full(3, 12345.0, np.float32)
    assert L.mse_explained_variance_host(values.size, _p(values), _p(returns), _p(out[1:])) == 0
    assert out[0] == 12345.0 and out[2] == 12345.0
    return out[1]


@pytest.mark.parametrize("n", EV_SIZES)
def test_explained_variance_host(n):
    L = M.load_library()
    values, returns = ev_inputs(n)
    got, want = ev_host(L, values, returns), ev_numpy(values, returns)
    if n == 1:
        assert math.isnan(got) and math.isnan(want)
    else:
        print(f"n={n}: host {got!r}, numpy float64 {want!r}, diff {abs(float(got) - want):.3e}")
        assert abs(float(got) - want) <= EV_BOUND * max(1.0, abs(want))
        assert ev_host(L, returns, returns) == 1.0  # values equal returns: exactly 1
        assert math.isnan(ev_host(L, values, np.full(n, 10.25, np.float32)))  # constant returns
        worse = ev_host(L, (-3 * values).astype(np.float32), returns)  # a critic that explains less than nothing
        w64 = ev_numpy((-3 * values).astype(np.float32), returns)
        assert worse < -1 and abs(float(worse) - w64) <= EV_BOUND * max(1.0, abs(w64))
    assert ev_host(L, values, returns).tobytes() == got.tobytes()


def test_explained_variance_abi_without_a_device():
    L = M.load_library()
    one = C.c_void_p(16)
    assert L.mse_explained_variance_workspace_bytes() == 256 * 4 * 8
    assert L.mse_explained_variance_workspace_bytes() <= L.mse_ppo_workspace_bytes(1, 1)  # the learner's workspace serves
    for args in ((0, one, one, one), (-1, one, one, one), (4, None, one, one), (4, one, None, one), (4, one, one, None)):
        assert L.mse_explained_variance_host(*args) == INVALID and b"mse_explained_variance_host" in L.mse_last_error()
        assert L.mse_explained_variance(*args, one, None) == INVALID and b"mse_explained_variance:" in L.mse_last_error()
    assert L.mse_explained_variance(4, one, one, one, None, None) == INVALID and b"workspace" in L.mse_last_error()
    assert L.mse_explained_variance(4, one, one, one, C.c_void_p(20), None) == ALIGNMENT
    if not torch.cuda.is_available():
        assert L.mse_explained_variance(4, one, one, one, one, None) == NO_DEVICE
