"""Exhaustive CPU proofs of the cheap quotient forms the step kernels use (marl-sortingenv_amd/csrc/mse_exact.h,
DESIGN.md 4.2): the integer purity hundredths for every 1 <= tru <= total <= kPurityExactMax, and the state reward's
reciprocal form for the shipped container capacity and the config-fuzz range.  The header is compiled on the host
as it is, and its results are compared with numpy's evaluation of the reference's literal expressions."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "marl-sortingenv_amd", "csrc")

SHIM = r"""
#include "mse_exact.h"
#include <math.h>
using namespace mse;
extern "C" {
unsigned purity_exact_max() { return kPurityExactMax; }
float purity_rcp_host(unsigned total) { return purity_rcp(total); }
// q and tie of purity_quotient for pairs (tru[i], total[i]) with the reciprocal moved by `ulps` units in the last place
void purity_batch(const int *tru, const int *total, long n, int ulps, int *q, unsigned char *tie)
{
    for (long i = 0; i < n; ++i) {
        float r = purity_rcp((unsigned)total[i]);
        for (int k = 0; k < ulps; ++k) r = nextafterf(r, INFINITY);
        for (int k = 0; k > ulps; --k) r = nextafterf(r, 0.0f);
        bool t;
        q[i] = (int)purity_quotient((unsigned)tru[i], (unsigned)total[i], r, t);
        tie[i] = t;
    }
}
void purity_literal_batch(const int *tru, const int *total, long n, int *q)
{
    for (long i = 0; i < n; ++i) q[i] = purity_literal(tru[i], total[i]);
}
void ratio_batch(const int *t, long n, double den, double inv, double *out)
{
    for (long i = 0; i < n; ++i) out[i] = ratio_by_reciprocal(t[i], den, inv);
}
int ratio_upto(double den, double inv, int limit) { return ratio_exact_upto(den, inv, limit); }
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler to build the mse_exact.h proof shim")
    d = tmp_path_factory.mktemp("exact")
    src, so = d / "shim.cpp", d / "shim.so"
    src.write_text(SHIM)
    # the kernels' flags for fp64: separately rounded operations, no fast math
    subprocess.run([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-I", CSRC,
                    str(src), "-o", str(so)], check=True)
    L = C.CDLL(str(so))
    L.purity_exact_max.restype = C.c_uint
    L.purity_rcp_host.restype = C.c_float
    L.purity_rcp_host.argtypes = [C.c_uint]
    L.ratio_upto.restype = C.c_int
    L.ratio_upto.argtypes = [C.c_double, C.c_double, C.c_int]
    return L


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _pairs(lo, hi):
    """every (tru, total) with lo <= total < hi and 0 <= tru <= total"""
    total = np.repeat(np.arange(lo, hi, dtype=np.int32), np.arange(lo, hi) + 1)
    start = np.repeat(np.cumsum(np.arange(lo, hi) + 1) - (np.arange(lo, hi) + 1), np.arange(lo, hi) + 1)
    tru = (np.arange(total.size) - start).astype(np.int32)
    return tru, total


def test_purity_bound_matches_header(lib):
    text = open(os.path.join(CSRC, "mse_exact.h")).read()
    assert int(re.search(r"kPurityExactMax = (\d+);", text).group(1)) == lib.purity_exact_max()
    # N = 200 tru + total must stay below 2^24 (exact in f32, a 24-bit multiply on the device)
    assert 201 * lib.purity_exact_max() < 1 << 24


def test_purity_integer_form_exhaustive(lib):
    """Every pair up to the bound, with the f32 reciprocal correctly rounded and one ulp either side (v_rcp_f32's
    accuracy): truncation gives floor((200 tru + total) / (2 total)) exactly, `tie` is set exactly at the halfway
    cases, and away from them the result is numpy's rint((tru / total) * 100)."""
    top = int(lib.purity_exact_max())
    n_ties = n_tie_diff = 0
    edges = np.unique(np.linspace(1, top + 1, 33).astype(np.int64))
    for lo, hi in zip(edges[:-1], edges[1:]):
        tru, total = _pairs(int(lo), int(hi))
        N = 200 * tru.astype(np.int64) + total
        D = 2 * total.astype(np.int64)
        exact_q = N // D
        exact_tie = N % D == 0
        literal = np.rint((tru / total) * 100.0).astype(np.int64)
        assert np.array_equal(literal[~exact_tie], exact_q[~exact_tie])
        for ulps in (-1, 0, 1):
            q = np.empty_like(tru)
            tie = np.empty(tru.size, np.uint8)
            lib.purity_batch(_ptr(tru), _ptr(total), C.c_long(tru.size), ulps, _ptr(q), _ptr(tie))
            assert np.array_equal(q, exact_q), (lo, hi, ulps)
            assert np.array_equal(tie.astype(bool), exact_tie), (lo, hi, ulps)
        # the literal fallback of the header is the reference's expression
        lit = np.empty_like(tru)
        lib.purity_literal_batch(_ptr(tru), _ptr(total), C.c_long(tru.size), _ptr(lit))
        assert np.array_equal(lit, literal)
        n_ties += int(exact_tie.sum())
        half_even = exact_q - ((exact_q & 1) == 1)  # at a tie q = rounded up; half-even takes the even neighbour
        n_tie_diff += int((literal[exact_tie] != half_even[exact_tie]).sum())
    # the ties do occur, and numpy's fp64 result is not half-even at all of them: they need the literal form
    assert n_ties > 0 and n_tie_diff > 0


def test_purity_reciprocal_is_within_one_ulp(lib):
    for total in (1, 3, 7, 700, 1454, 8192):
        r = np.float32(lib.purity_rcp_host(total))
        assert abs(float(r) - 1.0 / (2 * total)) <= float(np.spacing(r))


@pytest.mark.parametrize("capacity", [700, *range(300, 1200)])
def test_state_ratio_reciprocal_form(lib, capacity):
    """mse_create's proof for the shipped capacity and every capacity the config fuzz draws: the reciprocal form
    equals numpy's t / (5 capacity) for every total level a stepped env can hold (capacity + one batch of 255 per
    container), and ratio_exact_upto reports that whole range."""
    den = float(5 * capacity)
    inv = 1.0 / den
    limit = 5 * (capacity + 255)
    t = np.arange(limit + 1, dtype=np.int32)
    out = np.empty(t.size, np.float64)
    lib.ratio_batch(_ptr(t), C.c_long(t.size), C.c_double(den), C.c_double(inv), _ptr(out))
    literal = t / den
    assert np.array_equal(out.view(np.uint64), literal.view(np.uint64))
    assert lib.ratio_upto(den, inv, limit) == limit


def test_state_ratio_proof_finds_a_mismatch(lib):
    """The host proof is not vacuous: a plain product t * (1/D) differs from t / D (4 906 of 10 241 totals at
    D = 3 500), and a reciprocal off by a relative 1e-6 makes the corrected form fail."""
    den = 3500.0
    t = np.arange(10241)
    assert int(((t * (1.0 / den)) != (t / den)).sum()) > 1000
    bad_inv = (1.0 / den) * (1 + 1e-6)
    assert lib.ratio_upto(den, float(bad_inv), 10240) < 10240
