"""Host checks of tests/policy_head_reference.py: the register order, the kernel selector, the committed extreme-draw
indices and the float32 restatement of the sampler on a uniform policy."""
import numpy as np
import pytest

from tests import policy_head_reference as R
from tests import policy_stream as ps


@pytest.mark.parametrize("A", range(1, 33))
def test_register_order_is_a_permutation(A):
    order = R.register_order(A)
    assert sorted(order) == list(range(A))
    halves = [R.half_of(a) for a in order]
    assert halves == sorted(halves)  # half 0's rows first
    for h in (0, 1):
        rows = [a for a in order if R.half_of(a) == h]
        assert rows == sorted(rows) == [a for a in range(A) if (a >> 2) & 1 == h]


def test_regs_for_actions_and_selector_edges():
    assert [R.regs_for_actions(A) for A in (1, 2, 3, 4, 5, 8, 9, 11, 12, 16, 17, 22, 24, 25, 32)] == \
        [1, 2, 3, 4, 4, 4, 5, 7, 8, 8, 9, 12, 12, 13, 16]
    nr = {A: R.kernel_regs(A) for A in range(1, 33)}
    assert set(nr.values()) == set(R.KERNEL_REGS)
    assert (nr[1], nr[2], nr[3]) == (2, 2, 7)
    assert (nr[11], nr[12]) == (7, 12)
    assert (nr[24], nr[25], nr[32]) == (12, 16, 16)
    assert all(nr[A] <= nr[A + 1] for A in range(1, 32))
    # every register the kernel walks beyond the existing rows is a phantom: no row < A
    for A in range(1, 33):
        assert all(R.row_of(r, h) >= A for h in (0, 1) for r in range(R.regs_for_actions(A), nr[A]))


def test_extreme_draw_constants_have_the_words_they_claim():
    for idx in R.U_ZERO_INDICES:
        assert int(ps.word(R.EXTREME_SEED, np.array([idx]), R.EXTREME_T)[0]) >> 8 == 0
    for idx in R.U_MAX_INDICES:
        assert int(ps.word(R.EXTREME_SEED, np.array([idx]), R.EXTREME_T)[0]) >> 8 == 0xFFFFFF
    assert float(ps.uniform24(np.array([0xFFFFFF00]))[0]) == 1.0 - 2.0 ** -24


def _masks(A, n, seed):
    rng = np.random.default_rng(seed)
    mask = rng.random((n, A)) < 0.6
    mask[np.arange(n), rng.integers(0, A, n)] = True
    return mask


@pytest.mark.parametrize("A", [1, 2, 3, 11, 12, 22, 25, 32])
def test_uniform_sample_picks_legal_actions_and_the_ends_at_extreme_draws(A):
    n = 512
    mask = _masks(A, n, seed=A)
    words = ps.word(9, np.arange(n), 1)
    act = R.uniform_sample_f32(words, mask, A)
    assert ((act >= 0) & (act < A)).all() and mask[np.arange(n), act].all()
    lo = R.uniform_sample_f32(np.zeros(n, dtype=np.uint64), mask, A)
    hi = R.uniform_sample_f32(np.full(n, 0xFFFFFFFF, dtype=np.uint64), mask, A)
    hi2 = R.uniform_sample_f32(np.full(n, 0xFFFFFF00, dtype=np.uint64), mask, A)
    assert lo.tolist() == [R.first_legal_register(m, A) for m in mask]
    assert hi.tolist() == hi2.tolist() == [R.last_legal_register(m, A) for m in mask]
    # the low eight bits of the word are not used
    assert (R.uniform_sample_f32(words | np.uint64(0xFF), mask, A) == R.uniform_sample_f32(words & np.uint64(0xFFFFFF00), mask, A)).all()
    # the selector's NR and a wider one (more phantom registers) give the same action
    assert (R.uniform_sample_f32(words, mask, A, NR=16) == act).all()


@pytest.mark.parametrize("A,illegal", [(2, []), (11, [0, 10]), (22, [3, 7, 20]), (32, [0, 4, 27, 31])])
def test_uniform_sample_frequencies_are_uniform(A, illegal):
    n = 1 << 16
    mask = np.ones((n, A), dtype=bool)
    mask[:, illegal] = False
    act = R.uniform_sample_f32(ps.word(31, np.arange(n), 4), mask, A)
    freq = np.bincount(act, minlength=A) / n
    k = A - len(illegal)
    assert freq[illegal].sum() == 0.0
    assert np.abs(freq[mask[0]] - 1.0 / k).max() < 4.0 * np.sqrt((1.0 / k) * (1.0 - 1.0 / k) / n)


def test_uniform_sample_walks_in_register_order():
    """Every 24-bit draw of a small exhaustive grid: the action is the register-order entry floor(u * count), up to the
    one float32 rounding of u * count."""
    A = 22
    order = np.asarray(R.register_order(A))
    u24 = np.arange(0, 1 << 24, 4099, dtype=np.uint64)
    act = R.uniform_sample_f32(u24 << np.uint64(8), None, A)
    k = (u24.astype(np.float64) * 2.0 ** -24 * A)
    exact = order[np.floor(k).astype(np.int64)]
    off = act != exact
    assert (np.abs(k[off] - np.round(k[off])) < 2e-6).all() and off.mean() < 1e-3


def test_first_argmax_is_the_lowest_index_of_a_tie():
    lg = np.zeros((3, 6))
    lg[1, [2, 4]] = 1.0
    lg[2, [0, 5]] = 1.0
    mask = np.ones((3, 6), dtype=bool)
    assert R.first_argmax(lg).tolist() == [0, 2, 0]
    mask[2, 0] = False
    mask[0, :3] = False
    assert R.first_argmax(lg, mask).tolist() == [3, 2, 5]
