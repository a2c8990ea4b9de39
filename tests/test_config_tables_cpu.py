"""The config compiler (marl-sortingenv_amd/csrc/mse_tables.h) pinned on the CPU.  The header is compiled on the host as
it is, and every Params field and every word of the table image it makes is compared with the numpy / Python
restatement in tests/config_tables_reference.py: the default config, the fuzzed configs of test_oracle_config_fuzz.py,
the general generator mode, the `literal` rule, the image's structure and every refusal."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import marl_sortingenv_amd as M
from tests import config_tables_reference as R
from tests.fuzz_configs import fuzz_overrides

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "marl-sortingenv_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")
IMAGE_LIMIT = 16384  # words: 64 KiB

SHIM = r"""
#include "mse_tables.h"
using namespace mse;
extern "C" {
int sizeof_params() { return (int)sizeof(Params); }
int in_range(const mse_config *c, char *why, int why_len)
{
    const char *w = nullptr;
    const int rc = config_in_range(*c, w);
    why[0] = 0;
    if (w != nullptr) strncpy(why, w, why_len - 1);
    return rc;
}
int compile(const mse_config *c, long long n_envs, long long index_offset, Params *P, unsigned *image, int image_cap,
            int *words, int *literal, int *noise_on, char *why, int why_len)
{
    CompiledConfig cc;
    std::string w;
    const int rc = compile_config(*c, n_envs, index_offset, cc, w);
    why[0] = 0;
    strncpy(why, w.c_str(), why_len - 1);
    if (rc != MSE_OK) return rc;
    if ((int)cc.image.size() > image_cap) return 1000;
    *P = cc.P;
    memcpy(image, cc.image.data(), cc.image.size() * 4);
    *words = (int)cc.image.size();
    *literal = cc.literal;
    *noise_on = cc.noise_on;
    return rc;
}
void ratios(int n, double den, double inv, double *out)
{
    for (int t = 0; t < n; ++t) out[t] = ratio_by_reciprocal(t, den, inv);
}
}
"""

_INT, _U32 = C.c_int, C.c_uint32


class Params(C.Structure):  # csrc/mse_params.h
    _fields_ = [("n", C.c_longlong), ("n_pad", C.c_longlong), ("index_offset", C.c_longlong)] + \
               [(f, _INT) for f in ("env_kind", "max_steps", "auto_reset", "track_bales", "balesize", "capacity",
                                    "stage_capacity", "batch")] + \
               [("press_time", _INT * 2), ("press_time0", _INT), ("press_time1", _INT), ("inv_balesize", C.c_float),
                ("max_state_reward", C.c_double), ("sr_den", C.c_double), ("sr_inv", C.c_double), ("sr_exact_max", _INT),
                ("pat_word", _U32 * 3), ("pat_word1", _U32), ("pat_word2", _U32)] + \
               [(f, _INT) for f in ("thr_sev", "thr_mild", "sev_negative", "mild_negative")] + [("k_thr", _INT * 4)] + \
               [(f, _INT) for f in ("off_lvl", "off_pdiff", "off_timer0", "off_timer1", "off_tanh", "off_eff", "off_pat",
                                    "off_acc", "off_bonus", "off_ptime", "off_cst", "off_jump", "off_back",
                                    "table_words")] + \
               [("qi_down", _U32 * 4), ("rem_thr_units", _INT), ("ring_worst", _INT), ("ring_fwd", C.c_uint64 * 4),
                ("gen_mode", _INT), ("gen_rem", _INT * 3), ("occ_nonempty", _U32), ("off_gprop", _INT),
                ("off_gfrac", _INT), ("acc_floor", C.c_double * 4)]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler to build the mse_tables.h shim")
    d = tmp_path_factory.mktemp("tables")
    src, so = d / "shim.cpp", d / "shim.so"
    src.write_text(SHIM)
    subprocess.run([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-I", CSRC,
                    "-I", INCLUDE, str(src), "-o", str(so)], check=True)
    L = C.CDLL(str(so))
    L.in_range.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    L.compile.argtypes = [C.c_void_p, C.c_longlong, C.c_longlong, C.POINTER(Params), C.POINTER(C.c_uint32), C.c_int,
                          C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_char_p, C.c_int]
    L.ratios.argtypes = [C.c_int, C.c_double, C.c_double, C.POINTER(C.c_double)]
    assert L.sizeof_params() == C.sizeof(Params)
    return L


def compile_config(L, c, n_envs=1000, index_offset=0):
    """mse_create's order: the range checks, then the compiler.  -> (status, message, Params, image, literal, noise_on)"""
    why = C.create_string_buffer(512)
    rc = L.in_range(C.byref(c), why, 512)
    if rc != R.OK:
        return rc, why.value.decode(), None, None, None, None
    P, image = Params(), (C.c_uint32 * IMAGE_LIMIT)()
    words, literal, noise_on = C.c_int(), C.c_int(), C.c_int()
    rc = L.compile(C.byref(c), n_envs, index_offset, C.byref(P), image, IMAGE_LIMIT, C.byref(words), C.byref(literal),
                   C.byref(noise_on), why, 512)
    if rc != R.OK:
        return rc, why.value.decode(), None, None, None, None
    return rc, None, P, list(image[:words.value]), bool(literal.value), bool(noise_on.value)


def reference(c, n_envs=1000, index_offset=0):
    rc, why = R.config_in_range(c)
    return (rc, why, None, None, None, None) if rc != R.OK else R.compile_config(c, n_envs, index_offset)


def _same(a, b):
    """equal, floats by their bits"""
    if isinstance(b, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(b, (float, np.floating)):
        return np.asarray(a).tobytes() == np.asarray(b).tobytes() and np.asarray(a).dtype == np.asarray(b).dtype
    return int(a) == int(b)


def _field(P, name):
    v = getattr(P, name)
    if isinstance(v, C.Array):
        return list(v)
    kind = dict(Params._fields_)[name]
    return np.float32(v) if kind is C.c_float else (float(v) if kind is C.c_double else v)


def check(L, c, n_envs=1000, index_offset=0):
    """compile c both ways; every field, every word and both flags agree.  -> (Params, image, literal, noise_on)"""
    rc, why, P, image, literal, noise_on = compile_config(L, c, n_envs, index_offset)
    want_rc, want_why, want_P, want_image, want_literal, want_noise_on = reference(c, n_envs, index_offset)
    assert (rc, why) == (want_rc, want_why)
    assert rc == R.OK
    assert set(want_P) | {"sr_exact_max"} == {f for f, _ in Params._fields_}  # the restatement covers every field
    for name, want in want_P.items():
        assert _same(_field(P, name), want), (name, _field(P, name), want)
    assert len(image) == len(want_image) == P.table_words
    diff = [i for i, (a, b) in enumerate(zip(image, want_image)) if a != b]
    sections = sorted((getattr(P, f), f) for f, _ in Params._fields_ if f.startswith("off_"))
    assert not diff, [(i, max(s for s in sections if s[0] <= i)[1], hex(image[i]), hex(want_image[i])) for i in diff[:8]]
    assert (literal, noise_on) == (want_literal, want_noise_on)
    # sr_exact_max by property: the reciprocal form equals the division up to it and, below the limit, not at the next t
    limit = 5 * (c.container_capacity + 255)
    assert -1 <= P.sr_exact_max <= limit
    n = min(P.sr_exact_max + 2, limit + 1)
    got = (C.c_double * n)()
    L.ratios(n, P.sr_den, P.sr_inv, got)
    exact = np.array(got) == np.arange(n, dtype=np.float64) / P.sr_den
    assert exact[:P.sr_exact_max + 1].all()
    assert P.sr_exact_max == limit or not exact[P.sr_exact_max + 1]
    return P, image, literal, noise_on


def fuzzed(kind, seed):
    ov, ctor = fuzz_overrides(seed)
    return M.SortingEnvConfig().with_overrides(ov).to_struct(kind, **ctor)


@pytest.mark.parametrize("noise", (0.0, 0.05))
@pytest.mark.parametrize("kind", ("sort", "press", "mono"))
def test_default_config(lib, kind, noise):
    P, _, literal, noise_on = check(lib, M.SortingEnvConfig().to_struct(kind, noise_sorting=noise))
    assert (P.gen_mode, literal, noise_on) == (0, False, noise != 0.0)
    assert (P.n, P.n_pad, P.index_offset) == (1000, 1024, 0)


def test_sharded_handle(lib):
    P, *_ = check(lib, M.SortingEnvConfig().to_struct("mono"), n_envs=65536, index_offset=3 * 65536)
    assert (P.n, P.n_pad, P.index_offset) == (65536, 65536, 196608)


# the seeds of test_oracle_config_fuzz.py: every kind for the first six, mono for the rest
@pytest.mark.parametrize("kind,seed", [(k, s) for s in range(30) for k in (("sort", "press", "mono") if s < 6 else ("mono",))])
def test_fuzzed_config(lib, kind, seed):
    check(lib, fuzzed(kind, seed))


@pytest.mark.parametrize("batch", (90, 77))
def test_general_generator_mode(lib, batch):
    P, image, _, _ = check(lib, M.SortingEnvConfig(input_batch_size=batch).to_struct("mono"))
    ratios = M.SortingEnvConfig().pattern_ratios
    assert P.gen_mode == 1
    assert list(P.gen_rem) == [0] + [batch - sum(math.floor(r * batch) for r in ratios[k]) for k in range(2)]
    assert max(P.gen_rem) > 0
    assert P.off_gprop == P.off_back + 33 * 8 and P.off_gfrac == P.off_gprop + 256
    assert P.table_words == P.off_gfrac + 256


def test_empty_container_difference_is_rounded_by_python(lib):
    """pdiff[m][101] is Python's round of a Python float where a filled container's entries are numpy's round of an
    np.float64; a threshold of 0.005 is the one with at most three decimals where the two rounds of
    round(thr, 2) - thr differ (0.01 against 0.0), so it tells the two apart"""
    thr = 0.005
    d = round(thr, 2) - thr
    assert np.float32(round(d, 2)) != np.float32(round(np.float64(d), 2))
    P, image, _, _ = check(lib, M.SortingEnvConfig(bale_quality_thresholds=(thr, 0.9, 0.9, 0.9)).to_struct("mono"))
    assert image[P.off_pdiff + 101] == R.f32_words(0.01)[0]


@pytest.mark.parametrize("batch,literal_choice,want", [(127, False, False), (128, False, True), (255, False, True),
                                                       (100, True, True)])
def test_literal_rule(lib, batch, literal_choice, want):
    c = M.SortingEnvConfig(input_batch_size=batch, stage_capacity=255).to_struct("mono", literal_choice=literal_choice)
    assert check(lib, c)[2] is want


def _maps(image, at, count):
    """[(a, g)] of `count` LCG maps stored as A_lo A_hi G_lo G_hi u64s"""
    u64 = [image[at + 2 * i] | (image[at + 2 * i + 1] << 32) for i in range(4 * count)]
    return [(u64[4 * i] | (u64[4 * i + 1] << 64), u64[4 * i + 2] | (u64[4 * i + 3] << 64)) for i in range(count)]


def _steps(s, inc, n):
    for _ in range(n):
        s = (R.PCG_MULT * s + inc) & R.MASK128
    return s


@pytest.mark.parametrize("c", [lambda: M.SortingEnvConfig().to_struct("mono", noise_sorting=0.0),
                               lambda: M.SortingEnvConfig(input_batch_size=90).to_struct("press"),
                               lambda: fuzzed("mono", 3)])
def test_image_structure(lib, c):
    P, image, _, _ = check(lib, c())
    assert P.off_tanh % 2 == 0
    assert P.off_pat % 4 == 0 and P.off_jump % 4 == 0 and P.table_words % 4 == 0
    assert P.table_words <= IMAGE_LIMIT
    s, inc = 0x0123456789ABCDEF0F1E2D3C4B5A6978, 0xFEDCBA9876543210A5A5A5A5DEADBEEF | 1
    # jump entry j is the step map raised to the power 2^j: entry 0 is one step, entry j + 1 is entry j twice, and the
    # low entries agree with stepping
    jump = _maps(image, P.off_jump, R.JUMP_BITS)
    assert jump[0] == (R.PCG_MULT, 1)
    for j in range(R.JUMP_BITS - 1):
        assert jump[j + 1] == ((jump[j][0] * jump[j][0]) & R.MASK128, (jump[j][0] * jump[j][1] + jump[j][1]) & R.MASK128)
    for j in range(12):
        assert R.lcg_apply(jump[j], s, inc) == _steps(s, inc, 1 << j)
    # back entry d, composed with d forward steps, is the identity
    back = _maps(image, P.off_back, R.BACK_STEPS)
    for d in range(R.BACK_STEPS):
        assert R.lcg_apply(back[d], _steps(s, inc, d), inc) == s
    # ring_fwd is the step map raised to the power ring_worst
    fwd = (P.ring_fwd[0] | (P.ring_fwd[1] << 64), P.ring_fwd[2] | (P.ring_fwd[3] << 64))
    assert P.ring_worst > 0 and R.lcg_apply(fwd, s, inc) == _steps(s, inc, P.ring_worst)


def _default(**changes):
    c = M.SortingEnvConfig().to_struct("mono")
    for name, value in changes.items():
        if isinstance(value, tuple):
            for i, v in enumerate(value):
                getattr(c, name)[i] = v
        else:
            setattr(c, name, value)
    return c


def _same_patterns():
    c = _default()
    for m in range(4):
        c.pattern_ratio[1][m] = c.pattern_ratio[0][m]
    return c


# Every message of config_in_range and compile_config but one: "int(q*100) is not q or q-1" guards a property of the
# fp64 arithmetic itself ((q / 100.0) * 100.0 lands within one unit below q for q = 0..100), which no config can
# change and IEEE doubles satisfy, so there is nothing to feed the compiler that reaches it.
REFUSALS = [
    ("env_kind 0", lambda: _default(env_kind=0), R.INVALID_ARGUMENT, R.MSG_KIND),
    ("env_kind 4", lambda: _default(env_kind=4), R.INVALID_ARGUMENT, R.MSG_KIND),
    ("max_steps 0", lambda: _default(max_steps=0), R.UNSUPPORTED, R.MSG_MAX_STEPS),
    ("max_steps 65536", lambda: _default(max_steps=65536), R.UNSUPPORTED, R.MSG_MAX_STEPS),
    ("batch 0", lambda: _default(input_batch_size=0), R.UNSUPPORTED, R.MSG_BATCH),
    ("batch 256", lambda: _default(input_batch_size=256), R.UNSUPPORTED, R.MSG_BATCH),
    ("press_time 0", lambda: _default(press_time=(0, 15)), R.UNSUPPORTED, R.MSG_PRESS),
    ("press_time 256", lambda: _default(press_time=(12, 256)), R.UNSUPPORTED, R.MSG_PRESS),
    ("bale size 0", lambda: _default(bale_standard_size=0), R.UNSUPPORTED, R.MSG_SIZES),
    ("capacity 0", lambda: _default(container_capacity=0), R.UNSUPPORTED, R.MSG_SIZES),
    ("stage capacity 0", lambda: _default(stage_capacity=0), R.UNSUPPORTED, R.MSG_SIZES),
    ("noise negative", lambda: _default(noise=-0.01), R.UNSUPPORTED, R.MSG_NOISE),
    ("noise NaN", lambda: _default(noise=float("nan")), R.UNSUPPORTED, R.MSG_NOISE),
    ("identical patterns", _same_patterns, R.UNSUPPORTED, R.MSG_PATTERNS),
    ("threshold above 1", lambda: _default(quality_threshold_r2=(0.9, 1.01, 0.9, 0.9)), R.UNSUPPORTED, R.MSG_THRESHOLDS),
    ("threshold below 0", lambda: _default(quality_threshold_r2=(0.9, 0.9, 0.9, -0.01)), R.UNSUPPORTED, R.MSG_THRESHOLDS),
    ("image over 64 KiB", lambda: _default(container_capacity=12000, bale_standard_size=3000), R.UNSUPPORTED, R.MSG_IMAGE),
]


@pytest.mark.parametrize("name,config,status,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusal(lib, name, config, status, message):
    c = config()
    assert compile_config(lib, c)[:2] == (status, message)
    assert reference(c)[:2] == (status, message)


def test_refusals_cover_every_message():
    """each refusal the header can produce is in REFUSALS, but for the one no config reaches"""
    text = open(os.path.join(CSRC, "mse_tables.h")).read()
    messages = set(re.findall(r'why = "([^"]+)"', text))
    assert len(messages) == 10
    assert messages - {r[3] for r in REFUSALS} == {"int(q*100) is not q or q-1"}


def test_refusals_keep_their_order(lib):
    """the first failing check names the refusal: range checks in their order, then the compiler's"""
    c = _default(env_kind=0, max_steps=0, input_batch_size=0, noise=-1.0)
    assert compile_config(lib, c)[:2] == (R.INVALID_ARGUMENT, R.MSG_KIND)
    c.env_kind = 3
    assert compile_config(lib, c)[:2] == (R.UNSUPPORTED, R.MSG_MAX_STEPS)
    c.max_steps = 50
    assert compile_config(lib, c)[:2] == (R.UNSUPPORTED, R.MSG_BATCH)
    c = _same_patterns()
    c.quality_threshold_r2[0] = 2.0
    c.container_capacity, c.bale_standard_size = 12000, 3000
    assert compile_config(lib, c)[:2] == (R.UNSUPPORTED, R.MSG_PATTERNS)
    c = _default(container_capacity=12000, bale_standard_size=3000)
    c.quality_threshold_r2[0] = 2.0
    assert compile_config(lib, c)[:2] == (R.UNSUPPORTED, R.MSG_THRESHOLDS)
