"""CPU checks of PPO with an auxiliary imitation term: the head arithmetic, the ABI's refusals and the learner's
arguments (no device needed).

marl-sortingenv_amd/csrc/mse_ppo_math.h is compiled on the host as it is, through the shim below, which composes
policy_bc_head_terms (and value_head_terms / value_head_terms_clipped) row by row the way the KICK entries of the gradient
kernels do - the construction of tests/test_bc_math_cpu.py.  It is held against tests/ppo_bc_reference.py: float64 autograd
under the tolerance rule of tests/ppo_reference.py, the two counts exactly."""
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
from tests import bc_reference as B
from tests import ppo_bc_reference as K
from tests import ppo_reference as R
from tests.ppo_checks import DIM_MATRIX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "marl-sortingenv_amd", "csrc")
INVALID, ALIGNMENT = -1, -6

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

// a minibatch as k_ppo_grad_kick<DP, AP, VCLIP> composes it (old_values != NULL: VCLIP)
template <int DP, int AP>
static void run(int D, int A, const float *wflat, long B, const float *obs, const unsigned char *mask, const int *act,
                const float *old_logp, const float *adv, const float *ret, const float *old_values, const int *expert, Params P,
                float bc_coef, float *grad, double *stats)
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
    double sums[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (long b = 0; b < B; ++b) {
        float x[DP];
        for (int i = 0; i < DP; ++i) x[i] = i < D ? obs[b * D + i] : 0.0f;
        unsigned legal = 0;
        for (int a = 0; a < A; ++a) legal |= (mask == nullptr || mask[b * A + a] ? 1u : 0u) << a;
        const float a_used = normalize ? normalized_advantage(adv[b], mean, std) : adv[b];
        const int action = act[b] < 0 ? 0 : (act[b] >= A ? A - 1 : act[b]); // clamped_action of mse_ppo_grad.h
        float h1[kH], h2[kH], dz2[kH], dz1[kH], dl[AP];
        hidden_forward<DP>(&w[PW::pi_w1], &w[PW::pi_b1], &w[PW::pi_w2], &w[PW::pi_b2], x, h1, h2);
        head_forward<AP>(&w[PW::act_w], &w[PW::act_b], h2, dl);
        const PolicyBcTerms t = policy_bc_head_terms<AP>(dl, A, legal, action, expert[b], old_logp[b], a_used, P, bc_coef, inv_b);
        sums[0] += t.surrogate; sums[2] += t.entropy; sums[3] += t.kl; sums[4] += t.clipped;
        sums[5] += t.ce; sums[6] += t.hit; sums[7] += t.unusable;
        outer<kH>(&g[PW::act_w], &g[PW::act_b], dl, AP, h2, kH);
        backprop<AP>(&w[PW::act_w], dl, h2, dz2);
        outer<kH>(&g[PW::pi_w2], &g[PW::pi_b2], dz2, kH, h1, kH);
        backprop<kH>(&w[PW::pi_w2], dz2, h1, dz1);
        outer<DP>(&g[PW::pi_w1], &g[PW::pi_b1], dz1, kH, x, DP);
        hidden_forward<DP>(&w[PW::vf_w1], &w[PW::vf_b1], &w[PW::vf_w2], &w[PW::vf_b2], x, h1, h2);
        float v[1], dv[1];
        head_forward<1>(&w[PW::val_w], &w[PW::val_b], h2, v);
        sums[1] += old_values != nullptr ? value_head_terms_clipped(v[0], old_values[b], ret[b], P, inv_b, dv[0])
                                         : value_head_terms(v[0], ret[b], P, inv_b, dv[0]);
        outer<kH>(&g[PW::val_w], &g[PW::val_b], dv, 1, h2, kH);
        backprop<1>(&w[PW::val_w], dv, h2, dz2);
        outer<kH>(&g[PW::vf_w2], &g[PW::vf_b2], dz2, kH, h1, kH);
        backprop<kH>(&w[PW::vf_w2], dz2, h1, dz1);
        outer<DP>(&g[PW::vf_w1], &g[PW::vf_b1], dz1, kH, x, DP);
    }
    for (int f = 0; f < F.total; ++f) grad[f] = g[padded_index<DP, AP>(f, D, A)];
    const double pl = sums[0] / B, vl = sums[1] / B, el = -sums[2] / B, bl = sums[5] / B;
    stats[0] = pl + P.ent_coef * el + P.vf_coef * vl + (double)bc_coef * bl; stats[1] = pl; stats[2] = vl; stats[3] = el;
    stats[4] = sums[3] / B; stats[5] = sums[4] / B; stats[6] = mean; stats[7] = std;
    stats[8] = bl; stats[9] = (float)(sums[6] / B); stats[10] = (float)(sums[7] / B); stats[11] = 0.0;
}

extern "C" {
int kick_rows(int D, int A, const float *wflat, long B, const float *obs, const unsigned char *mask, const int *act,
              const float *old_logp, const float *adv, const float *ret, const float *old_values, const int *expert, float clip,
              float ent, float vf, int norm, float clip_vf, float bc_coef, float *grad, double *stats)
{
    Params P{clip, ent, vf, norm, clip_vf};
    const GradShape shape = select_grad_shape(D, A);
    if (shape == kShapeNone) return -1;
#define SHIM_RUN(DP, AP) run<DP, AP>(D, A, wflat, B, obs, mask, act, old_logp, adv, ret, old_values, expert, P, bc_coef, grad, stats)
    MSE_PPO_DISPATCH(shape, SHIM_RUN);
#undef SHIM_RUN
    return 0;
}

// one row's head at AP = 32, both ways: d_* receive the gradients w.r.t. the logits, t_* the terms
// (plain: surrogate, entropy, kl, clipped, logp;  kick: the same five, then ce, hit, unusable)
void head_pair(int A, const float *logits, unsigned legal, int action, int expert, float old_logp, float adv, float clip, float ent,
               float bc_coef, float inv_b, float *d_plain, float *t_plain, float *d_kick, float *t_kick)
{
    Params P{clip, ent, 0.5f, 1};
    float a[32], b[32];
    for (int i = 0; i < 32; ++i) a[i] = b[i] = i < A ? logits[i] : 0.0f;
    const PolicyTerms p = policy_head_terms<32>(a, A, legal, action, old_logp, adv, P, inv_b);
    const PolicyBcTerms k = policy_bc_head_terms<32>(b, A, legal, action, expert, old_logp, adv, P, bc_coef, inv_b);
    for (int i = 0; i < 32; ++i) { d_plain[i] = a[i]; d_kick[i] = b[i]; }
    t_plain[0] = p.surrogate; t_plain[1] = p.entropy; t_plain[2] = p.kl; t_plain[3] = p.clipped; t_plain[4] = p.logp;
    t_kick[0] = k.surrogate; t_kick[1] = k.entropy; t_kick[2] = k.kl; t_kick[3] = k.clipped; t_kick[4] = k.logp;
    t_kick[5] = k.ce; t_kick[6] = k.hit; t_kick[7] = k.unusable;
}
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler to build the mse_ppo_math.h shim")
    d = tmp_path_factory.mktemp("ppo_bc")
    src, so = d / "shim.cpp", d / "shim.so"
    src.write_text(SHIM)
    subprocess.run([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-I", CSRC,
                    str(src), "-o", str(so)], check=True)
    L = C.CDLL(str(so))
    L.head_pair.restype = None
    L.head_pair.argtypes = [C.c_int, C.c_void_p, C.c_uint, C.c_int, C.c_int] + [C.c_float] * 6 + [C.c_void_p] * 4
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def run_shim(shim, D, A, flat, rows, bc_coef, normalize=True, hp=K.HP):
    n = rows["obs"].shape[0]
    grad = np.zeros(R.num_weights(D, A), np.float32)
    stats = np.zeros(12, np.float64)
    m8 = None if rows["mk"] is None else np.ascontiguousarray(rows["mk"].numpy().astype(np.uint8))
    old = None if rows["old"] is None else rows["old"].numpy()
    rc = shim.kick_rows(D, A, _p(flat.numpy()), C.c_long(n), _p(np.ascontiguousarray(rows["obs"].numpy())), _p(m8),
                        _p(rows["actions"].numpy()), _p(rows["old_logp"].numpy()), _p(rows["adv"].numpy()), _p(rows["ret"].numpy()),
                        _p(old), _p(rows["labels"].numpy()), C.c_float(hp["clip_range"]), C.c_float(hp["ent_coef"]),
                        C.c_float(hp["vf_coef"]), int(normalize), C.c_float(K.C_VF if old is not None else 0.0), C.c_float(bc_coef),
                        _p(grad), _p(stats))
    assert rc == 0
    return torch.from_numpy(grad), torch.from_numpy(stats)


@pytest.mark.parametrize("with_old", [False, True])
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("D,A", DIM_MATRIX)
def test_header_four_term_loss_and_gradient_match_float64_autograd(shim, D, A, masked, with_old):
    flat = R.random_flat(D, A, seed=D * 100 + A)
    rows = K.make_kick_rows(D, A, 300, 17, flat, masked, with_old)
    K.assert_margins(flat, D, A, rows)
    for bc_coef in K.BC_COEFS:
        ref = K.reference(flat, D, A, rows, bc_coef)
        g, s = run_shim(shim, D, A, flat, rows, bc_coef)
        K.check(f"header {D}->{A} masked={masked} old_values={with_old} bc_coef={bc_coef}", g, s, ref)
    s64 = ref[1]
    if A > 1:
        assert 0.3 < float(s64[9]) < 1.0  # hits and misses both occur
    if masked and A > 1:
        assert float(s64[10]) > 0.0  # ... and so do unusable rows


def head_pair(shim, A, logits, legal, action, expert, old_logp=-1.0, adv=0.7, bc_coef=0.0, inv_b=1.0 / 64):
    lg = np.ascontiguousarray(np.asarray(logits, np.float32))
    out = [np.zeros(32, np.float32), np.zeros(5, np.float32), np.zeros(32, np.float32), np.zeros(8, np.float32)]
    shim.head_pair(A, _p(lg), legal, action, expert, old_logp, adv, K.HP["clip_range"], K.HP["ent_coef"], bc_coef, inv_b,
                   *[_p(o) for o in out])
    return out


def _random_heads(n, seed):
    g = np.random.default_rng(seed)
    for _ in range(n):
        A = int(g.integers(1, 33))
        legal = int(g.integers(1, 2 ** A)) | 1
        logits = (g.standard_normal(A) * 3.0).astype(np.float32)
        ok = [a for a in range(A) if (legal >> a) & 1]
        yield A, logits, legal, int(g.choice(ok)), int(g.integers(0, A)), float(-g.random() * 3.0), float(g.standard_normal() * 1.5)


def test_bc_coef_zero_equals_the_ppo_head_on_every_term(shim):
    """the middle summand is +-0: every d[a] and every PPO term equals policy_head_terms' under =="""
    n_unusable = 0
    for A, logits, legal, action, expert, old_logp, adv in _random_heads(400, 3):
        d0, t0, d1, t1 = head_pair(shim, A, logits, legal, action, expert, old_logp, adv, bc_coef=0.0)
        assert np.all(d0 == d1), (A, legal, action, expert)
        assert np.all(t0 == t1[:5])
        n_unusable += int(t1[7])
        # ... and with a coefficient the PPO terms still do; only the gradient moves, and only on a usable row
        d2, t2 = head_pair(shim, A, logits, legal, action, expert, old_logp, adv, bc_coef=0.5)[2:]
        assert np.all(t0 == t2[:5]) and np.all(t1[5:] == t2[5:])
        if t2[7] == 1.0:
            assert np.all(d0 == d2)
    assert 20 < n_unusable < 380  # both branches were taken


def test_label_equal_to_the_action_taken(shim):
    """both one-hots sit on one logit: d = (g_logp + g_bc) (onehot - p) + entropy term, within rounding of the two products"""
    for A, logits, legal, action, _, old_logp, adv in _random_heads(100, 5):
        inv_b, c = 1.0 / 64, 0.5
        d0, t0, d1, t1 = head_pair(shim, A, logits, legal, action, action, old_logp, adv, bc_coef=c, inv_b=inv_b)
        assert t1[7] == 0.0 and t1[5] == -t1[4]  # usable (the action is legal), and ce is -logp of that action, exactly
        lp = np.full(A, -np.inf)
        ok = np.array([(legal >> a) & 1 for a in range(A)], bool)
        x = logits.astype(np.float64)[ok]
        lp[ok] = x - (x.max() + np.log(np.exp(x - x.max()).sum()))
        p = np.exp(lp)
        onehot = (np.arange(A) == action).astype(np.float64)
        want = d0[:A].astype(np.float64) - c * inv_b * (onehot - p)
        # three more float32 roundings than d0 has (the product, its sum, the entropy term's sum), each half an ulp of an
        # intermediate no larger than |g_logp| + c inv_b + the entropy term (ent_coef inv_b (|lp| + 1 + rest) < 8 ent_coef inv_b
        # here); p itself carries a few ulp.  8 ulp of that magnitude covers both.
        size = abs(adv) * math.exp(float(t0[4]) - old_logp) * inv_b + c * inv_b + 8 * K.HP["ent_coef"] * inv_b
        assert np.all(np.abs(d1[:A] - np.where(ok, want, 0.0)) <= 8 * np.finfo(np.float32).eps * size)


def test_an_illegal_label_keeps_the_ppo_and_entropy_terms_and_counts_as_unusable(shim):
    D, A = 29, 22
    flat = R.random_flat(D, A, seed=9)
    rows = K.make_kick_rows(D, A, 64, 23, flat, True)
    rows["mask"][:, A - 1] = False
    rows["mask"][:, 1] = True
    rows["actions"] = torch.where(rows["actions"] == A - 1, torch.zeros_like(rows["actions"]), rows["actions"])  # stay legal
    rows["mk"] = rows["mask"]
    rows["labels"] = torch.full((64,), A - 1, dtype=torch.int32)  # every label is illegal
    g, s = run_shim(shim, D, A, flat, rows, 4.0)
    K.check("illegal labels", g, s, K.reference(flat, D, A, rows, 4.0))
    assert float(s[8]) == 0.0 and float(s[9]) == 0.0 and float(s[10]) == 1.0
    g0, s0 = run_shim(shim, D, A, flat, rows, 0.0)  # nothing of the imitation term is left: the gradient is PPO's
    assert np.array_equal(g.numpy(), g0.numpy()) and np.array_equal(s.numpy()[:8], s0.numpy()[:8])
    assert float(s[3]) < 0.0 and float(s[1]) != 0.0
    # labels outside the head are clamped into it first: A + 7 is A - 1, illegal here; -3 is 0, legal
    for raw, unusable in ((A + 7, 1.0), (-3, 0.0), (2 ** 31 - 1, 1.0), (-2 ** 31, 0.0)):
        rows["labels"] = torch.full((64,), raw, dtype=torch.int32)
        g2, s2 = run_shim(shim, D, A, flat, rows, 0.5)
        clamped = dict(rows, labels=rows["labels"].clamp(0, A - 1))
        K.check(f"label {raw} clamped", g2, s2, K.reference(flat, D, A, clamped, 0.5))
        assert float(s2[10]) == unusable


@pytest.mark.parametrize("D,A", [(29, 22), (13, 2)])
def test_one_hot_mask_rows(shim, D, A):
    """every row has one legal action: p = 1 there, ce = 0, and the actor's gradient vanishes whatever the coefficient"""
    flat = R.random_flat(D, A, seed=3)
    rows = K.make_kick_rows(D, A, 40, 2, flat, True)
    only = torch.arange(40) % A
    mask = torch.zeros((40, A), dtype=torch.bool)
    mask[torch.arange(40), only] = True
    rows.update(mask=mask, mk=mask, actions=only.int(), labels=only.int(), old_logp=torch.zeros(40))
    g, s = run_shim(shim, D, A, flat, rows, 4.0)
    assert float(s[8]) == 0.0 and float(s[9]) == 1.0 and float(s[10]) == 0.0 and float(s[3]) == 0.0
    assert float(g[:B.critic_slice(D, A).start].abs().max()) == 0.0
    rows["labels"] = ((only + 1) % A).int()  # ... and an illegal label changes nothing but the counts
    g2, s2 = run_shim(shim, D, A, flat, rows, 4.0)
    assert np.array_equal(g.numpy(), g2.numpy()) and float(s2[9]) == 0.0 and float(s2[10]) == 1.0


@pytest.mark.parametrize("A", [6, 22, 32])
def test_exact_ties_go_to_the_lowest_index(shim, A):
    second = 4
    legal = (1 << 2) | (1 << second) | (1 << (A - 1))
    logits = np.full(A, 0.25, np.float32)
    lowest = min(second, 2)
    for expert in (2, second, A - 1):
        t = head_pair(shim, A, logits, legal, 2, expert, bc_coef=1.0)[3]
        assert t[6] == (1.0 if expert == lowest else 0.0) and t[7] == 0.0
        assert abs(float(t[5]) - math.log(3.0)) < 1e-6  # three equal legal logits
    for expert, hit in ((0, 1.0), (1, 0.0)):  # unmasked: the winner is action 0
        assert head_pair(shim, A, logits, 2 ** A - 1, 0, expert, bc_coef=1.0)[3][6] == hit


def test_abi_refusals_without_a_device():
    L = M.load_library()
    for name in ("mse_ppo_bc_loss_grad", "mse_ppo_bc_workspace_bytes"):
        assert hasattr(L, name) and name in EXPORTS
    assert L.mse_ppo_bc_workspace_bytes(0, 2) == 0 and L.mse_ppo_bc_workspace_bytes(29, 33) == 0
    assert L.mse_ppo_bc_workspace_bytes(29, 22) >= L.mse_ppo_workspace_bytes(29, 22) > 0
    one = C.c_void_p(16)  # a non-null pointer that is never followed: every call below fails its argument checks
    p = MsePpoParams(C.sizeof(MsePpoParams), 0.2, 0.0, 0.5, 1)
    #     0   1   2    3   4     5   6    7     8    9    10   11   12           13   14   15   16    17   18    19 20   21   22   23
    ok = [29, 22, one, 64, None, 64, one, None, one, one, one, one, C.byref(p), one, one, one, None, 0.0, None, 0, one, 0.2, one, 0.5]

    def call(**change):
        a = list(ok)
        for k, v in change.items():
            a[int(k[1:])] = v
        return L.mse_ppo_bc_loss_grad(*a)

    def why():
        return L.mse_last_error()

    # mse_ppo_loss_grad_vclip's checks, in its order
    assert call(a17=float("nan"), a18=one) == INVALID and b"mse_ppo_bc_loss_grad: target_kl is NaN" in why()
    for i in (2, 6, 8, 9, 10, 11, 12, 13, 14, 15):
        assert call(**{f"a{i}": None}) == INVALID and b"mse_ppo_bc_loss_grad: null argument" in why(), i
    assert call(a0=0) == INVALID and b"1..32" in why()
    assert call(a1=33) == INVALID
    bad = MsePpoParams(3, 0.2, 0.0, 0.5, 1)
    assert call(a12=C.byref(bad)) == INVALID and b"struct_size" in why()
    assert call(a3=0) == INVALID and b"batch" in why()
    assert call(a5=65) == INVALID  # batch > n_rows without rows_dev
    nan = MsePpoParams(C.sizeof(MsePpoParams), 0.2, float("nan"), 0.5, 1)
    assert call(a12=C.byref(nan)) == INVALID and b"ent_coef" in why()
    assert call(a15=C.c_void_p(24)) == ALIGNMENT and b"16-byte aligned" in why()
    assert call(a19=2) == INVALID and b"arithmetic" in why()
    for c in (0.0, -0.1, float("nan"), float("inf"), 1e-60):
        assert call(a21=c) == INVALID and b"clip_range_vf" in why(), c
    # the new ones, after all of those
    assert call(a22=None) == INVALID and b"mse_ppo_bc_loss_grad: null expert_actions" in why()
    for c in (-0.5, float("nan"), float("inf"), float("-inf"), 1e300):  # 1e300 is finite, its float32 is not
        assert call(a23=c) == INVALID and b"bc_coef" in why(), c
    # the documented order: each check hides the ones after it
    assert call(a21=0.0, a22=None) == INVALID and b"clip_range_vf" in why()
    assert call(a19=2, a22=None) == INVALID and b"arithmetic" in why()
    assert call(a22=None, a23=-1.0) == INVALID and b"expert_actions" in why()
    assert call(a15=C.c_void_p(24), a23=-1.0) == ALIGNMENT
    # what passes every check reaches the device question: 0 and a float32 denormal are coefficients like any other
    for c in (0.0, 1e-45, 4.0):
        rc = call(a23=c, a20=None)
        assert rc != INVALID and rc != ALIGNMENT, (c, why())


def test_labelled_rollout_refusals_without_a_device():
    """what mse_rollout_policy_labelled and its check-only twin refuse before any handle is looked into"""
    L = M.load_library()
    for name in ("mse_rollout_policy_labelled", "mse_rollout_policy_labelled_check"):
        assert hasattr(L, name) and name in EXPORTS
    one = C.c_void_p(16)
    outs = [one] * 10
    for env, pol in ((None, None), (None, one), (one, None)):
        assert L.mse_rollout_policy_labelled_check(env, pol, 4, 7, 0, None, 0) == INVALID
        assert b"env/policy is NULL" in L.mse_last_error()
        assert L.mse_rollout_policy_labelled(env, pol, 4, 7, 0, None, 0, *outs, None) == INVALID
        assert b"env/policy is NULL" in L.mse_last_error()


class _Policy:
    """what PPOLearner's constructor validates its arguments before: nothing of a device"""


def test_learner_arguments_without_a_device():
    from types import SimpleNamespace

    from marl_sortingenv_amd.learner import PPO_BC_STAT_NAMES, STAT_NAMES, resolve_schedule

    assert STAT_NAMES == R.STAT_NAMES and PPO_BC_STAT_NAMES == K.STAT_NAMES and len(PPO_BC_STAT_NAMES) == 12
    assert M.PPO_BC_STAT_NAMES is PPO_BC_STAT_NAMES
    assert resolve_schedule(0.0, 1.0, "bc_coef", allow_zero=True) == 0.0
    assert resolve_schedule(lambda p: 2.0 * p, 0.25, "bc_coef", allow_zero=True) == 0.5
    for bad in (-1.0, float("nan"), float("inf"), lambda p: -p):
        with pytest.raises(ValueError, match="bc_coef"):
            M.PPOLearner(_Policy(), bc_coef=bad)  # refused before the policy is looked at
    # hyperparameters() names bc_coef only when it is set: as a value, or under `scheduled`
    fields = dict(policy=SimpleNamespace(obs_dim=29, n_actions=22), n_epochs=10, batch_size=None, gamma=0.99, gae_lambda=0.95,
                  params=MsePpoParams(C.sizeof(MsePpoParams), 0.2, 0.05, 0.5, 1), max_grad_norm=0.5, adam_eps=1e-5, beta1=0.9,
                  beta2=0.999, seed=0, shuffle="cpu", weight_sync="host", target_kl=None, arithmetic="fma", schedules={},
                  learning_rate=3e-4, clip_range=0.2, clip_range_vf=None)
    before = M.PPOLearner.hyperparameters(SimpleNamespace(**fields, bc_coef=None))
    assert "bc_coef" not in before and before["scheduled"] == []
    assert set(before) == {"obs_dim", "n_actions", "n_epochs", "batch_size", "gamma", "gae_lambda", "ent_coef", "vf_coef",
                           "max_grad_norm", "normalize_advantage", "adam_eps", "beta1", "beta2", "seed", "shuffle", "weight_sync",
                           "target_kl", "arithmetic", "scheduled", "learning_rate", "clip_range", "clip_range_vf"}
    assert M.PPOLearner.hyperparameters(SimpleNamespace(**fields, bc_coef=0.5)) == dict(before, bc_coef=0.5)
    fields["schedules"] = {"bc_coef": lambda p: p}
    assert M.PPOLearner.hyperparameters(SimpleNamespace(**fields, bc_coef=1.0)) == dict(before, scheduled=["bc_coef"])
