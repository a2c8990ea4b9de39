"""CPU checks of the demonstration rollout's mixture rule (no device needed): `mse_demo_who_steps_host`, which runs the
kernel's own inline function (csrc/mse_demo_mix.h), against a numpy restatement on tests/policy_stream.py; the public
`expert_threshold`; and the condition tests/test_gpu_demo_rollout.py's mixture tests stand on - at the seed, threshold
and sizes they use, both branches of "who steps" are taken about equally often."""
import ctypes as C

import numpy as np
import pytest

from tests import policy_stream as ps

ONE = 1 << 24
MIX_SEED = 99  # the mixture tests' (tests/test_gpu_demo_rollout.py)


def who_steps(n, index_offset, mix_seed, t, threshold):
    """u8[n]: 1 where the expert steps env index_offset + j at step counter t - the word of (mix_seed, global env index,
    t), its upper 24 bits compared with the integer threshold."""
    w = ps.word(mix_seed, np.arange(n, dtype=np.uint64) + np.uint64(index_offset), t)
    return ((w >> np.uint64(8)) < np.uint64(threshold)).astype(np.uint8)


@pytest.fixture(scope="module")
def lib():
    import marl_sortingenv_amd as M

    return M.load_library()


def _host(lib, n, index_offset, mix_seed, t, threshold):
    out = np.full(n + 2, 7, dtype=np.uint8)  # one guard byte on each side
    rc = lib.mse_demo_who_steps_host(n, index_offset, mix_seed, t, threshold, out[1:].ctypes.data_as(C.c_void_p))
    assert out[0] == 7 and out[-1] == 7
    return rc, out[1:-1]


@pytest.mark.parametrize("threshold", [0, 1, 1 << 23, ONE - 1, ONE])
def test_who_steps_host_equals_restatement(lib, threshold):
    n = 1000
    total = 0
    for index_offset in (0, 1, 4096, 2 ** 32 - 3, 2 ** 40 + 17):  # the last two: an index's upper word enters the key
        for mix_seed in (0, MIX_SEED, 2 ** 64 - 1):
            for t in (0, 1, 9, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 5, 2 ** 63 + 11):
                rc, got = _host(lib, n, index_offset, mix_seed, t, threshold)
                assert rc == 0
                want = who_steps(n, index_offset, mix_seed, t, threshold)
                assert np.array_equal(got, want), (index_offset, mix_seed, t)
                total += int(got.sum())
    cells = n * 5 * 3 * 7
    if threshold == 0:
        assert total == 0
    elif threshold == ONE:
        assert total == cells
    elif threshold == 1 << 23:
        assert 0.49 < total / cells < 0.51
    elif threshold == 1:
        assert total <= 3  # 105 000 words, each below 2^8 with probability 2^-24
    else:
        assert total >= cells - 3


def test_who_steps_depends_on_every_argument(lib):
    """The upper word of t and of the index, and the seed, each change the decisions (a restatement and a library that
    both dropped one of them would still agree with each other)."""
    n, thr = 512, 1 << 23
    base = _host(lib, n, 0, MIX_SEED, 5, thr)[1].copy()
    for args in ((0, MIX_SEED, 5 + 2 ** 32), (2 ** 32, MIX_SEED, 5), (0, MIX_SEED + 1, 5), (0, MIX_SEED + 2 ** 32, 5), (1, MIX_SEED, 5)):
        other = _host(lib, n, args[0], args[1], args[2], thr)[1]
        assert 0.3 < float((other != base).mean()) < 0.7, args
    # shifting the window by one env shifts the decisions by one
    assert np.array_equal(_host(lib, n, 1, MIX_SEED, 5, thr)[1][:-1], base[1:])


def test_who_steps_host_refusals(lib):
    INVALID = -1
    out = np.zeros(4, dtype=np.uint8)
    p = out.ctypes.data_as(C.c_void_p)
    assert lib.mse_demo_who_steps_host(4, 0, 1, 0, ONE + 1, p) == INVALID
    assert b"mse_demo_who_steps_host" in lib.mse_last_error()
    assert lib.mse_demo_who_steps_host(-1, 0, 1, 0, 5, p) == INVALID
    assert lib.mse_demo_who_steps_host(4, -1, 1, 0, 5, p) == INVALID
    assert lib.mse_demo_who_steps_host(4, 0, 1, 0, 5, None) == INVALID
    assert lib.mse_demo_who_steps_host(0, 0, 1, 0, 5, None) == 0
    assert not out.any()


def test_expert_threshold():
    from marl_sortingenv_amd.imitation import expert_threshold

    assert expert_threshold(0) == 0 and expert_threshold(0.0) == 0
    assert expert_threshold(1) == ONE and expert_threshold(1.0) == ONE
    assert expert_threshold(0.5) == 1 << 23
    assert expert_threshold(0.25) == 1 << 22
    assert expert_threshold(2.0 ** -24) == 1
    assert expert_threshold(2.0 ** -26) == 0  # rounds to nearest
    assert expert_threshold(1.0 - 2.0 ** -24) == ONE - 1
    assert expert_threshold(0.1) == int(round(0.1 * 2 ** 24)) == 1677722
    assert isinstance(expert_threshold(np.float32(0.5)), int)
    for bad in (float("nan"), -1e-9, 1.0 + 1e-9, -1, 2, float("inf"), float("-inf")):
        with pytest.raises(ValueError):
            expert_threshold(bad)
    import marl_sortingenv_amd as M

    assert M.expert_threshold is expert_threshold


@pytest.mark.parametrize("n, expect", [(33, 163), (257, 1265)])
def test_mixture_condition_of_the_gpu_tests(lib, n, expect):
    """mix_seed 99, threshold 2^23, index_offset 0, t = 0 .. 9: the expert's share is between 40 % and 60 %, so a GPU
    mixture test at these settings exercises both branches (163 / 330 and 1265 / 2570 rows)."""
    rows = np.stack([who_steps(n, 0, MIX_SEED, t, 1 << 23) for t in range(10)])
    for t in range(10):
        assert np.array_equal(_host(lib, n, 0, MIX_SEED, t, 1 << 23)[1], rows[t])
    share = rows.mean()
    print(f"n={n}: the expert steps {int(rows.sum())} of {rows.size} rows ({share:.3f})")
    assert 0.4 <= share <= 0.6
    assert int(rows.sum()) == expect
    assert rows.any(axis=0).sum() > 0 and (~rows.astype(bool)).any(axis=0).sum() > 0
