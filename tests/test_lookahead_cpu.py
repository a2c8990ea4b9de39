"""CPU checks of the lookahead planner (no device needed): `mse_lookahead_stream_seed` - the library's host entry point
and csrc/mse_lookahead_seed.h compiled as it is by the host compiler - against a numpy restatement of the header's
comment; the refusals of `mse_lookahead` that need no handle; and what `BatchedSortingEnv.lookahead`,
`LookaheadCollector` and `evaluate_lookahead` refuse in Python before anything is stepped."""
import ctypes as C
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "marl-sortingenv_amd", "csrc")
INVALID = -1

SEEDS = (0, 1, 2 ** 64 - 1)
INDICES = (0, 1, 65535, 2 ** 32 + 1)
SAMPLES = (0, 1, 7)
GOLDEN = np.uint64(0x9E3779B97F4A7C15)


def mix(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def stream_seed(seed, index, sample):
    """include/mse.h: a = mix(seed + G); b = mix(a ^ index); c = mix(b + (sample + 1) G); c >> 1 (modulo 2^64)."""
    with np.errstate(over="ignore"):
        a = mix(np.uint64(seed) + GOLDEN)
        b = mix(a ^ np.uint64(index))
        c = mix(b + (np.uint64(sample) + np.uint64(1)) * GOLDEN)
    return int(c >> np.uint64(1))


@pytest.fixture(scope="module")
def lib():
    import marl_sortingenv_amd as M

    return M.load_library()


@pytest.fixture(scope="module")
def header(tmp_path_factory):
    """csrc/mse_lookahead_seed.h as the host compiler sees it, behind one exported function."""
    d = tmp_path_factory.mktemp("lookahead_seed")
    src, so = d / "shim.cpp", d / "shim.so"
    src.write_text('#include "mse_lookahead_seed.h"\n'
                   'extern "C" unsigned long long seed_of(unsigned long long s, unsigned long long i, unsigned int m)\n'
                   "{ return mse_lookahead_seed_of(s, i, m); }\n")
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    subprocess.run([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(so)], check=True)
    L = C.CDLL(str(so))
    L.seed_of.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32]
    L.seed_of.restype = C.c_uint64
    return L


def test_stream_seed_equals_restatement(lib, header):
    seen = {}
    for seed in SEEDS:
        for index in INDICES:
            for sample in SAMPLES:
                want = stream_seed(seed, index, sample)
                assert int(lib.mse_lookahead_stream_seed(seed, index, sample)) == want, (seed, index, sample)
                assert int(header.seed_of(seed, index, sample)) == want, (seed, index, sample)
                assert 0 <= want < 2 ** 63  # a seed mse_reset's callers can carry as a signed integer; + 99 does not wrap
                seen[(seed, index, sample)] = want
    assert len(set(seen.values())) == len(seen) == 36


def test_stream_seed_depends_on_every_argument(lib):
    """The upper word of the seed and of the index and every bit of the sample enter (a restatement and a library that both
    dropped one would still agree with each other)."""
    base = int(lib.mse_lookahead_stream_seed(5, 9, 2))
    for args in ((5 + 2 ** 32, 9, 2), (5, 9 + 2 ** 32, 2), (5, 9, 2 + 2 ** 16), (6, 9, 2), (5, 10, 2), (5, 9, 3)):
        other = int(lib.mse_lookahead_stream_seed(*args))
        assert other != base and 8 <= bin(other ^ base).count("1") <= 56, args


def test_refusals_that_need_no_handle(lib):
    q = np.full(8, 7.0)
    ws = np.full(8, 7.0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    # a NULL env is the first refusal, whatever else is wrong
    assert lib.mse_lookahead(None, 4, 1.0, 1, 2024, 1, 0, 1, None, 0, p(q), None, None, p(ws), None) == INVALID
    assert b"mse_lookahead" in lib.mse_last_error()
    assert lib.mse_lookahead(None, 0, 2.0, 5, 0, 5, 0, 0, None, 255, None, None, None, None, None) == INVALID
    assert int(lib.mse_lookahead_workspace_bytes(None, 1)) == INVALID
    assert (q == 7.0).all() and (ws == 7.0).all()


def _fake_env(**over):
    base = dict(auto_reset=True, obs_dim=29, num_actions=22, num_envs=4, kind="mono")
    return types.SimpleNamespace(**dict(base, **over))


def test_lookahead_refuses_in_python_before_the_library():
    from marl_sortingenv_amd.batched import BatchedSortingEnv

    env = _fake_env()  # no handle: a refusal that came later than these would raise AttributeError instead
    with pytest.raises(ValueError, match="base_policy"):
        BatchedSortingEnv.lookahead(env, 4, base_policy="greedy")
    with pytest.raises(ValueError, match="streams"):
        BatchedSortingEnv.lookahead(env, 4, streams="new")
    for h in (0, -3):
        with pytest.raises(ValueError, match="horizon"):
            BatchedSortingEnv.lookahead(env, h)
    with pytest.raises(ValueError, match="n_samples"):
        BatchedSortingEnv.lookahead(env, 4, n_samples=0)


def test_collector_and_evaluation_refusals():
    import marl_sortingenv_amd as M
    from marl_sortingenv_amd.lookahead import LookaheadCollector, evaluate_lookahead

    assert M.LookaheadCollector is LookaheadCollector and M.evaluate_lookahead is evaluate_lookahead
    assert callable(M.lookahead_reference)
    for name in ("lookahead_reference", "LookaheadCollector", "evaluate_lookahead"):
        assert name in M.__all__
    env = _fake_env()
    with pytest.raises(ValueError, match="base_policy"):
        LookaheadCollector(env, 8, 4, base_policy="greedy")
    with pytest.raises(ValueError, match="streams"):
        LookaheadCollector(env, 8, 4, streams="mine")
    with pytest.raises(ValueError, match="horizon"):
        LookaheadCollector(env, 8, 0)
    with pytest.raises(ValueError, match="n_steps"):
        LookaheadCollector(env, 0, 4)
    with pytest.raises(TypeError, match="unknown lookahead argument"):
        LookaheadCollector(env, 8, 4, horizons=3)
    with pytest.raises(ValueError, match="auto_reset"):
        LookaheadCollector(_fake_env(auto_reset=False), 8, 4)
    for dims in ((16, 11), (29, 11), (13, 22)):
        actor = types.SimpleNamespace(obs_dim=dims[0], n_actions=dims[1])
        with pytest.raises(ValueError, match="29 -> 22"):
            LookaheadCollector(env, 8, 4, actor=actor)
    with pytest.raises(ValueError, match="streams"):
        evaluate_lookahead(env, 10, 4, streams="mine")
    with pytest.raises(ValueError, match="horizon"):
        evaluate_lookahead(env, 10, 0)
    with pytest.raises(ValueError, match="auto_reset"):
        evaluate_lookahead(_fake_env(auto_reset=False), 10, 4)
    with pytest.raises(ValueError, match="n_eval_episodes"):
        evaluate_lookahead(env, 0, 4)
