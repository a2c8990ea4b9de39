"""CPU checks of the learner's counter-based minibatch permutation (no device needed): `mse_ppo_shuffle_host`, which runs
the inline function of marl-sortingenv_amd/csrc/mse_ppo_math.h that `k_ppo_shuffle` runs, against
tests/ppo_shuffle_reference.py (numpy, written from the header's comment) bit for bit, and against what a shuffle has
to be: a bijection at every size, the same whatever windows it is asked for in, uniform in every position over seeds
and over epochs, and spreading the steps of a rollout evenly over the minibatches.  Every input is fixed, so the
statistical checks are deterministic; their bounds are quantiles of the exact laws, not measurements of this code."""
import ctypes as C

import numpy as np
import pytest

import marl_sortingenv_amd as M
from tests import ppo_shuffle_reference as S

SIZES = [1, 2, 3, 4, 5, 63, 64, 65, 4097, 65536, 65537, 2 ** 20 + 1]
# (seed, epoch): small, a seed above 2^32, an epoch above 2^32, all bits set
KEYS = [(0, 0), (5, 3), (2 ** 40 + 5, 1), (12345678901234567, 2 ** 33 + 9), (2 ** 64 - 1, 2 ** 64 - 1)]
INVALID = -1  # MSE_ERR_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def lib():
    return M.load_library()


def _call(lib, total, seed, epoch, first, count, out):
    return lib.mse_ppo_shuffle_host(total, seed, epoch, first, count, None if out is None else out.ctypes.data_as(C.c_void_p))


def host(lib, total, seed, epoch, first=0, count=None):
    count = total - first if count is None else count
    out = np.full(count, -7, np.int64)
    assert _call(lib, total, seed, epoch, first, count, out) == 0
    return out


@pytest.fixture(scope="module")
def whole(lib):
    """perm(seed = 5, epoch = 3) at every size, computed once."""
    return {total: host(lib, total, 5, 3) for total in SIZES}


@pytest.mark.parametrize("total", SIZES)
def test_bijection(whole, total):
    assert np.array_equal(np.sort(whole[total]), np.arange(total))


@pytest.mark.parametrize("total", SIZES)
def test_equal_to_the_restatement(lib, whole, total):
    for seed, epoch in KEYS:
        got = whole[total] if (seed, epoch) == (5, 3) else host(lib, total, seed, epoch)
        assert np.array_equal(got, S.permutation(total, seed, epoch)), (total, seed, epoch)


def test_both_halves_of_the_seed_and_the_epoch_matter(lib):
    base = host(lib, 4097, 5, 3)
    for seed, epoch in ((5 + 2 ** 32, 3), (5 + 2 ** 63, 3), (6, 3), (5, 4), (5, 3 + 2 ** 32)):
        other = host(lib, 4097, seed, epoch)
        assert np.mean(other == base) < 0.01, (seed, epoch)  # two random permutations agree in 1 of 4097 places


@pytest.mark.parametrize("total", [2 ** 31, 2 ** 31 - 1])
def test_large_total_by_window(lib, total):
    seen = []
    for first in (0, total - 4096):
        got = host(lib, total, 2 ** 40 + 5, 1, first, 4096)
        assert got.min() >= 0 and got.max() < total
        assert np.array_equal(got, S.permutation(total, 2 ** 40 + 5, 1, first, 4096))
        seen.append(got)
    assert np.unique(np.concatenate(seen)).size == 2 * 4096


@pytest.mark.parametrize("total", [1, 2, 5, 65, 4097, 65537])
def test_windows_concatenate_to_the_whole(lib, whole, total):
    rng = np.random.default_rng(total)
    for _ in range(4):
        cuts = np.sort(rng.integers(0, total + 1, size=min(7, total + 1)))  # repeated cuts give empty windows
        edges = [0, *cuts.tolist(), total]
        parts = [host(lib, total, 5, 3, a, b - a) for a, b in zip(edges[:-1], edges[1:])]
        assert np.array_equal(np.concatenate(parts), whole[total]), edges
    one_by_one = [host(lib, total, 5, 3, i, 1)[0] for i in range(min(total, 70))]
    assert one_by_one == whole[total][:70].tolist()


def test_count_zero_is_a_no_op(lib):
    out = np.full(4, -7, np.int64)
    for total, first in ((1, 0), (1, 1), (100, 50), (100, 100), (2 ** 31, 2 ** 31)):
        assert _call(lib, total, 5, 3, first, 0, out) == 0
        assert _call(lib, total, 5, 3, first, 0, None) == 0
    assert out.tolist() == [-7] * 4


@pytest.mark.parametrize("total,first,count,null", [
    (0, 0, 0, False), (-1, 0, 0, False), (2 ** 31 + 1, 0, 1, False), (2 ** 40, 0, 1, False),  # total outside 1 .. 2^31
    (100, -1, 1, False), (100, 0, -1, False), (100, 99, 2, False), (100, 101, 0, False), (100, 0, 101, False),
    (100, 2 ** 62, 2 ** 62, False), (100, 1, 2 ** 63 - 1, False),  # first + count past total, past int64 too
    (100, 0, 4, True),  # null output with count > 0
])
def test_invalid_arguments_are_refused_and_write_nothing(lib, total, first, count, null):
    out = np.full(8, -7, np.int64)
    assert _call(lib, total, 5, 3, first, count, None if null else out) == INVALID
    assert b"mse_ppo_shuffle_host" in lib.mse_last_error()
    assert out.tolist() == [-7] * 8


# ---- marginal uniformity -------------------------------------------------------------------------------------------------
# For every position i the value perm(i) should be uniform on [0, total) over keys.  The statistic is Pearson's chi-square of
# the S observed values against S / total each; the bounds are the 1 - 1e-6 quantiles of chi2(total - 1) (scipy.stats.chi2.ppf),
# so all `total` positions of a case pass together with probability 1 - total * 1e-6 under the exact law.  (Uniformity
# over whole permutations is not asked for: six Feistel rounds reach a small part of the total! permutations.)
CHI2_BOUND = {3: 27.64, 24: 70.55, 100: 180.80}


def _max_chi_square(lib, total, keys):
    counts = np.zeros((total, total), np.int64)
    out = np.empty(total, np.int64)
    at = np.arange(total)
    for seed, epoch in keys:
        assert _call(lib, total, seed, epoch, 0, total, out) == 0
        counts[at, out] += 1
    expected = len(keys) / total
    return float((((counts - expected) ** 2) / expected).sum(axis=1).max())


@pytest.mark.parametrize("total,n_seeds", [(3, 6000), (24, 20000), (100, 40000)])
def test_every_position_is_uniform_over_seeds(lib, total, n_seeds):
    worst = _max_chi_square(lib, total, [(s, s % 7) for s in range(n_seeds)])
    print(f"total {total}, seeds 0 .. {n_seeds - 1}, epoch = seed % 7: largest chi-square over positions {worst:.2f} "
          f"(bound {CHI2_BOUND[total]})")
    assert worst < CHI2_BOUND[total]


def test_every_position_is_uniform_over_epochs(lib):
    worst = _max_chi_square(lib, 100, [(77, e) for e in range(40000)])
    print(f"total 100, seed 77, epochs 0 .. 39999: largest chi-square over positions {worst:.2f} (bound {CHI2_BOUND[100]})")
    assert worst < CHI2_BOUND[100]


def test_minibatches_draw_evenly_from_every_step(lib):
    """2^16 rows = 16 steps x 4 096 envs, four minibatches: the rows of one step in one quarter follow a hypergeometric law
    (16 384 draws, 4 096 of 65 536 marked): mean 1 024, sigma = sqrt(16384 * 1/16 * 15/16 * 49152/65535) = 26.8; 6 sigma."""
    lo, hi = 10 ** 9, 0
    for seed, epoch in ((0, 0), (1, 0), (2 ** 40 + 5, 9)):
        step = host(lib, 2 ** 16, seed, epoch) // 4096
        for quarter in step.reshape(4, 16384):
            c = np.bincount(quarter, minlength=16)
            lo, hi = min(lo, int(c.min())), max(hi, int(c.max()))
    print(f"rows of one step in one quarter: {lo} .. {hi} (1024 +- 161 allowed)")
    assert 1024 - 161 <= lo and hi <= 1024 + 161
