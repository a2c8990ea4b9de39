"""CPU checks of the behaviour-cloning arithmetic and ABI (no device needed).

marl-sortingenv_amd/csrc/mse_ppo_math.h is compiled on the host as it is, through the shim below, which composes
bc_head_terms (and value_head_terms) row by row the way the behaviour-cloning instantiation of k_ppo_grad does, summing
the outer products in float32 - the construction of tests/test_ppo_math_cpu.py.  It is held against
tests/bc_reference.py: float64 autograd under the tolerance rule of tests/ppo_reference.py, the two counts exactly."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import marl_sortingenv_amd as M
from marl_sortingenv_amd._lib import EXPORTS, MsePpoParams
from tests import bc_reference as B
from tests import ppo_reference as R
from tests.ppo_checks import DIM_MATRIX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "marl-sortingenv_amd", "csrc")

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

template <int DP, int AP>
static void run(int D, int A, const float *wflat, long B, const float *obs, const unsigned char *mask, const int *act,
                const float *ret, Params P, float *grad, double *stats)
{
    typedef Padded<DP, AP> PW;
    const Flat F = flat_layout(D, A);
    std::vector<float> w(PW::total, 0.0f), g(PW::total, 0.0f);
    for (int f = 0; f < F.total; ++f) w[padded_index<DP, AP>(f, D, A)] = wflat[f];
    const float inv_b = 1.0f / (float)B;
    double sums[5] = {0, 0, 0, 0, 0};
    for (long b = 0; b < B; ++b) {
        float x[DP];
        for (int i = 0; i < DP; ++i) x[i] = i < D ? obs[b * D + i] : 0.0f;
        unsigned legal = 0;
        for (int a = 0; a < A; ++a) legal |= (mask == nullptr || mask[b * A + a] ? 1u : 0u) << a;
        float h1[kH], h2[kH], dz2[kH], dz1[kH], dl[AP];
        hidden_forward<DP>(&w[PW::pi_w1], &w[PW::pi_b1], &w[PW::pi_w2], &w[PW::pi_b2], x, h1, h2);
        head_forward<AP>(&w[PW::act_w], &w[PW::act_b], h2, dl);
        const BcTerms t = bc_head_terms<AP>(dl, A, legal, act[b], P, inv_b);
        sums[0] += t.ce; sums[2] += t.entropy; sums[3] += t.hit; sums[4] += t.unusable;
        outer<kH>(&g[PW::act_w], &g[PW::act_b], dl, AP, h2, kH);
        backprop<AP>(&w[PW::act_w], dl, h2, dz2);
        outer<kH>(&g[PW::pi_w2], &g[PW::pi_b2], dz2, kH, h1, kH);
        backprop<kH>(&w[PW::pi_w2], dz2, h1, dz1);
        outer<DP>(&g[PW::pi_w1], &g[PW::pi_b1], dz1, kH, x, DP);
        if (ret == nullptr) continue; // the critic contributes nothing
        hidden_forward<DP>(&w[PW::vf_w1], &w[PW::vf_b1], &w[PW::vf_w2], &w[PW::vf_b2], x, h1, h2);
        float v[1], dv[1];
        head_forward<1>(&w[PW::val_w], &w[PW::val_b], h2, v);
        sums[1] += value_head_terms(v[0], ret[b], P, inv_b, dv[0]);
        outer<kH>(&g[PW::val_w], &g[PW::val_b], dv, 1, h2, kH);
        backprop<1>(&w[PW::val_w], dv, h2, dz2);
        outer<kH>(&g[PW::vf_w2], &g[PW::vf_b2], dz2, kH, h1, kH);
        backprop<kH>(&w[PW::vf_w2], dz2, h1, dz1);
        outer<DP>(&g[PW::vf_w1], &g[PW::vf_b1], dz1, kH, x, DP);
    }
    for (int f = 0; f < F.total; ++f) grad[f] = g[padded_index<DP, AP>(f, D, A)];
    const double bl = sums[0] / B, vl = sums[1] / B, el = -sums[2] / B;
    stats[0] = bl + (double)P.ent_coef * el + (double)P.vf_coef * vl; stats[1] = bl; stats[2] = vl; stats[3] = el;
    stats[4] = (float)(sums[3] / B); stats[5] = (float)(sums[4] / B); stats[6] = 0.0; stats[7] = 1.0;
}

extern "C" int bc_rows(int D, int A, const float *wflat, long B, const float *obs, const unsigned char *mask, const int *act,
                       const float *ret, float ent, float vf, float *grad, double *stats)
{
    Params P{0.0f, ent, vf, 0};
    const GradShape shape = select_grad_shape(D, A);
    if (shape == kShapeNone) return -1;
#define SHIM_RUN(DP, AP) run<DP, AP>(D, A, wflat, B, obs, mask, act, ret, P, grad, stats)
    MSE_PPO_DISPATCH(shape, SHIM_RUN);
#undef SHIM_RUN
    return 0;
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler to build the mse_ppo_math.h shim")
    d = tmp_path_factory.mktemp("bc")
    src, so = d / "shim.cpp", d / "shim.so"
    src.write_text(SHIM)
    subprocess.run([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-I", CSRC,
                    str(src), "-o", str(so)], check=True)
    return C.CDLL(str(so))


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def run_shim(shim, D, A, flat, obs, mk, labels, ret, hp=B.HP):
    n = obs.shape[0]
    grad = np.zeros(R.num_weights(D, A), np.float32)
    stats = np.zeros(8, np.float64)
    m8 = None if mk is None else np.ascontiguousarray(mk.numpy().astype(np.uint8))
    r = None if ret is None else np.ascontiguousarray(ret.numpy())
    rc = shim.bc_rows(D, A, _p(flat.numpy()), C.c_long(n), _p(np.ascontiguousarray(obs.numpy())), _p(m8),
                      _p(np.ascontiguousarray(labels.numpy())), _p(r), C.c_float(hp["ent_coef"]), C.c_float(hp["vf_coef"]),
                      _p(grad), _p(stats))
    assert rc == 0
    return torch.from_numpy(grad), torch.from_numpy(stats)


@pytest.mark.parametrize("with_returns", [True, False])
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("D,A", DIM_MATRIX)
def test_header_bc_loss_and_gradient_match_float64_autograd(shim, D, A, masked, with_returns):
    flat = R.random_flat(D, A, seed=D * 100 + A)
    obs, mask, mk, labels, ret = B.make_bc_rows(D, A, 300, seed=17, flat=flat, masked=masked)
    B.assert_margins(flat, D, A, obs, mk)
    if masked:
        assert int(mask[0].sum()) == 1  # the one-hot mask row
    ret = ret if with_returns else None
    g, s = run_shim(shim, D, A, flat, obs, mk, labels, ret)
    _, s64 = B.check(f"header {D}->{A} masked={masked} returns={with_returns}", g, s, flat, D, A, obs, mk, labels, ret)
    if A > 1:
        assert 0.3 < float(s64[4]) < 1.0  # hits and misses both occur
    if masked and A > 1:
        assert float(s64[5]) > 0.0  # ... and so do unusable rows


def _tie_case(D, A, legal_idx, label):
    """an all-zero action head with equal biases: every logit is the bias, exactly, in any precision"""
    flat = R.random_flat(D, A, seed=5).clone()
    parts = R.split(flat, D, A)  # views into flat
    parts[4].zero_()
    parts[5].fill_(0.25)
    n = 6
    obs = torch.rand((n, D), generator=torch.Generator().manual_seed(1)) * 2.0 - 1.0
    mask = torch.zeros((n, A), dtype=torch.bool)
    mask[:, legal_idx] = True
    return flat, obs, mask, torch.full((n,), label, dtype=torch.int32)


@pytest.mark.parametrize("D,A", [(29, 22), (16, 11), (32, 32)])
def test_exact_ties_go_to_the_lowest_legal_action(shim, D, A):
    legal = [2, 5, A - 1]
    for label, hits in ((2, 1.0), (5, 0.0), (A - 1, 0.0)):
        flat, obs, mask, labels = _tie_case(D, A, legal, label)
        g, s = run_shim(shim, D, A, flat, obs, mask, labels, None)
        B.check(f"ties {D}->{A} label {label}", g, s, flat, D, A, obs, mask, labels, None)
        assert float(s[4]) == hits and float(s[5]) == 0.0
        assert abs(float(s[1]) - np.log(3.0)) < 1e-6  # three equal legal logits
    # unmasked: the winner is action 0
    for label, hits in ((0, 1.0), (1, 0.0)):
        flat, obs, mask, labels = _tie_case(D, A, list(range(A)), label)
        g, s = run_shim(shim, D, A, flat, obs, None, labels, None)
        assert float(s[4]) == hits


@pytest.mark.parametrize("D,A", [(29, 22), (13, 2)])
def test_one_hot_mask_rows(shim, D, A):
    """every row has one legal action: p = 1 there, ce = 0, the entropy and the actor's gradient vanish"""
    flat = R.random_flat(D, A, seed=3)
    n = 40
    obs = torch.rand((n, D), generator=torch.Generator().manual_seed(2)) * 2.0 - 1.0
    only = torch.arange(n) % A
    mask = torch.zeros((n, A), dtype=torch.bool)
    mask[torch.arange(n), only] = True
    g, s = run_shim(shim, D, A, flat, obs, mask, only.int(), None)
    B.check(f"one-hot {D}->{A}", g, s, flat, D, A, obs, mask, only.int(), None)
    assert float(s[1]) == 0.0 and float(s[3]) == 0.0 and float(s[4]) == 1.0 and float(s[5]) == 0.0
    assert float(g.abs().max()) == 0.0


@pytest.mark.parametrize("D,A", [(29, 22), (16, 11)])
def test_an_illegal_demonstration_teaches_nothing_but_keeps_its_entropy_term(shim, D, A):
    flat = R.random_flat(D, A, seed=9)
    def edit(mask):
        mask[:, 1] = True
        mask[:, A - 1] = False

    obs, mask, mk, labels, ret = B.make_bc_rows(D, A, 64, seed=23, flat=flat, masked=True, edit_mask=edit)
    B.assert_margins(flat, D, A, obs, mask)
    bad = torch.full((64,), A - 1, dtype=torch.int32)  # every demonstration is illegal
    g, s = run_shim(shim, D, A, flat, obs, mask, bad, None)
    g64, _ = B.check(f"illegal {D}->{A}", g, s, flat, D, A, obs, mask, bad, None)
    assert float(s[1]) == 0.0 and float(s[4]) == 0.0 and float(s[5]) == 1.0
    assert float(s[3]) < 0.0 and float(g.abs().max()) > 0.0  # the entropy term is still there ...
    # ... and is all there is: what the code was just held to is the gradient of ent_coef * entropy_loss alone
    other = torch.zeros(64, dtype=torch.int32)
    g_ent = B.loss_and_grad(flat, torch.float64, D, A, obs, mask, other, None, B.HP["ent_coef"], 0.0)[0] \
        - B.loss_and_grad(flat, torch.float64, D, A, obs, mask, other, None, 0.0, 0.0)[0]
    assert float((g64 - g_ent).abs().max()) <= 1e-12 * float(g_ent.abs().max())
    # actions outside the head are clamped into it first: A + 7 is A - 1, which is illegal here; -3 is 0, which is legal
    for raw, unusable in ((A + 7, 1.0), (-3, 0.0)):
        lab = torch.full((64,), raw, dtype=torch.int32)
        g2, s2 = run_shim(shim, D, A, flat, obs, mask, lab, None)
        B.check(f"clamped {raw} {D}->{A}", g2, s2, flat, D, A, obs, mask, lab, None)
        assert float(s2[5]) == unusable


def test_without_returns_the_critic_gradient_is_exactly_zero(shim):
    D, A = 29, 22
    flat = R.random_flat(D, A, seed=11)
    obs, mask, mk, labels, ret = B.make_bc_rows(D, A, 100, seed=29, flat=flat, masked=True)
    g0, s0 = run_shim(shim, D, A, flat, obs, mk, labels, None)
    g1, s1 = run_shim(shim, D, A, flat, obs, mk, labels, ret)
    cs = B.critic_slice(D, A)
    assert bool((g0[cs] == 0).all()) and float(s0[2]) == 0.0
    assert float(g1[cs].abs().max()) > 0.0 and float(s1[2]) > 0.0
    actor = slice(0, cs.start)
    assert np.array_equal(g0[actor].numpy().view(np.uint32), g1[actor].numpy().view(np.uint32))  # the actor does not see returns
    assert float(s0[1]) == float(s1[1]) and float(s0[3]) == float(s1[3])


def test_bc_abi_refusals_without_a_device():
    L = M.load_library()
    assert hasattr(L, "mse_bc_loss_grad") and "mse_bc_loss_grad" in EXPORTS
    INVALID, ALIGNMENT = -1, -6
    one = C.c_void_p(16)  # a non-null pointer that is never followed: every call below fails its argument checks
    p = MsePpoParams(C.sizeof(MsePpoParams), 0.2, 0.0, 0.5, 1)
    #     0   1   2    3   4     5   6    7     8    9     10           11   12   13   14    15
    ok = [29, 22, one, 64, None, 64, one, None, one, None, C.byref(p), one, one, one, None, 0]

    def call(**change):
        a = list(ok)
        for k, v in change.items():
            a[int(k[1:])] = v
        return L.mse_bc_loss_grad(*a)

    def why():
        return L.mse_last_error()

    for i in (2, 6, 8, 10, 11, 12, 13):  # weights, obs, actions, params, grad_out, stats_out, workspace
        assert call(**{f"a{i}": None}) == INVALID and b"mse_bc_loss_grad: null argument" in why(), i
    assert call(a0=0) == INVALID and b"1..32" in why()
    assert call(a0=33) == INVALID and call(a1=0) == INVALID and call(a1=33) == INVALID
    bad = MsePpoParams(3, 0.2, 0.0, 0.5, 1)
    assert call(a10=C.byref(bad)) == INVALID and b"struct_size" in why()
    assert call(a3=0) == INVALID and b"batch" in why()
    assert call(a3=-1) == INVALID and call(a5=0) == INVALID
    assert call(a5=65) == INVALID  # batch > n_rows without rows_dev
    for ent, vf in ((float("inf"), 0.5), (float("nan"), 0.5), (0.0, float("-inf")), (0.0, float("nan"))):
        refused = MsePpoParams(C.sizeof(MsePpoParams), 0.2, ent, vf, 1)
        assert call(a10=C.byref(refused)) == INVALID and b"ent_coef" in why(), (ent, vf)
    # clip_range and normalize_advantage are ignored: values mse_ppo_loss_grad refuses get past the argument checks here
    # (the next refusal, the workspace's alignment, shows it - no device is asked)
    for clip in (-0.1, float("nan")):
        ignored = MsePpoParams(C.sizeof(MsePpoParams), clip, 0.0, 0.5, 7)
        assert call(a10=C.byref(ignored), a13=C.c_void_p(24)) == ALIGNMENT
    for off in (8, 4, 1):
        assert call(a13=C.c_void_p(16 + off)) == ALIGNMENT and b"16-byte aligned" in why()
    for arithmetic in (2, -1):
        assert call(a15=arithmetic) == INVALID and b"arithmetic" in why()
    # the documented order: each check hides the ones after it
    assert call(a2=None, a0=0) == INVALID and b"null argument" in why()
    assert call(a0=0, a10=C.byref(bad)) == INVALID and b"1..32" in why()
    assert call(a10=C.byref(bad), a5=0) == INVALID and b"struct_size" in why()
    nan = MsePpoParams(C.sizeof(MsePpoParams), 0.2, float("nan"), 0.5, 1)
    assert call(a5=0, a10=C.byref(nan)) == INVALID and b"batch" in why()
    assert call(a10=C.byref(nan), a13=C.c_void_p(24)) == INVALID and b"ent_coef" in why()
    assert call(a13=C.c_void_p(24), a15=2) == ALIGNMENT


def test_imitation_front_end_is_exported():
    assert M.ImitationLearner is not None and M.DemonstrationCollector is not None
    assert issubclass(M.ImitationLearner, M.PPOLearner)
    from marl_sortingenv_amd.imitation import BC_STAT_NAMES

    assert BC_STAT_NAMES[:6] == B.STAT_NAMES[:6] and len(BC_STAT_NAMES) == 8
