"""CPU checks of the episode accounting (no device needed): `mse_episode_scan_host` and `mse_episode_summary_host`, which
run the inline functions of marl-sortingenv_amd/csrc/mse_episode_math.h that the kernels run, against
tests/episode_reference.py (numpy, written from the header's comment and SB3's counting rule).  Per-env outputs
(ledger returns as float64 bit patterns, lengths, counts, carry), the episode count, the length sum, min and max are
exact; the return sum, mean and std are held against math.fsum-based values within the bounds derived in DESIGN.md
4.13 (tests/episode_reference.py restates them) - nothing is taken from the code under test."""
import ctypes as C
import math

import numpy as np
import pytest

import marl_sortingenv_amd as M
from tests import episode_reference as R

INVALID = -1  # MSE_ERR_INVALID_ARGUMENT
SIZES = [1, 2, 63, 64, 65, 257]
STEPS = [1, 2, 16, 33]
PATTERNS = ["none", "all", "first", "last", "bernoulli"]


@pytest.fixture(scope="module")
def lib():
    return M.load_library()


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def make_ends(pattern, K, n, rng):
    ends = np.zeros((K, n), bool)
    if pattern == "all":
        ends[:] = True
    elif pattern == "first":
        ends[0] = True
    elif pattern == "last":
        ends[K - 1] = True
    elif pattern == "bernoulli":
        ends = rng.random((K, n)) < 0.1
    return ends


def make_rewards(K, n, rng):
    """float32 of mixed sign over five orders of magnitude, so that the double sums round"""
    return (rng.standard_normal((K, n)) * 10.0 ** rng.integers(-3, 2, (K, n))).astype(np.float32)


class Host:
    """Caller-owned arrays of one accounting, the ledger between two guard rows"""

    def __init__(self, n, slots=0, targets=None, totals=True):
        self.n, self.slots = n, slots
        self.run_return, self.run_length = np.zeros(n, np.float64), np.zeros(n, np.int32)
        self.ep_count = np.zeros(n, np.int32)
        self.targets = None if targets is None else np.ascontiguousarray(targets, np.int32)
        self._lr = np.full((slots + 2, n), np.nan, np.float64)
        self._ll = np.full((slots + 2, n), -1, np.int32)
        self.ledger_return = self._lr[1:slots + 1] if slots else None
        self.ledger_length = self._ll[1:slots + 1] if slots else None
        self.totals = np.zeros(5, np.float64) if totals else None

    def scan(self, lib, rewards, ends, form, first_row=None):
        K, n = rewards.shape
        if form == "dones":
            d, s, l = np.ascontiguousarray(ends, np.uint8), None, None
        else:
            s, l = R.starts_from_ends(ends, np.ones(n, np.uint8) if first_row is None else first_row)
            d = None
        return lib.mse_episode_scan_host(K, n, _p(rewards), _p(d), _p(s), _p(l), _p(self.run_return), _p(self.run_length),
                                         _p(self.ep_count), _p(self.targets), self.slots, _p(self.ledger_return),
                                         _p(self.ledger_length), _p(self.totals))

    def summary(self, lib):
        out = np.full(6, -7.0)
        assert lib.mse_episode_summary_host(self.n, self.slots, _p(self.ep_count), _p(self.ledger_return), _p(self.ledger_length),
                                            _p(out)) == 0
        return out

    def guards_intact(self):
        return (np.isnan(self._lr[[0, -1]]).all() and (self._ll[[0, -1]] == -1).all())


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def check_per_env(h, ref, label):
    assert same_bits(h.run_return, ref.run_return), label
    assert np.array_equal(h.run_length, ref.run_length), label
    assert np.array_equal(h.ep_count, ref.ep_count), label
    if h.slots:
        assert same_bits(h.ledger_return, ref.ledger_return), label  # NaN cells of episodes that did not happen included
        assert np.array_equal(h.ledger_length, ref.ledger_length), label
        assert h.guards_intact(), label


def check_totals(totals, counted, label):
    """count, length sum, min and max exactly; the return sum within (count - 1) 2^-53 sum|return| of math.fsum"""
    rets = [c[0] for c in counted]
    assert totals[0] == len(counted) and totals[2] == sum(c[1] for c in counted), label
    if not counted:
        assert totals.tolist() == [0.0] * 5, label
        return
    assert totals[3] == min(rets) and totals[4] == max(rets), label
    err, bound = abs(totals[1] - R.exact_sum(rets)), R.sum_bound(rets)
    assert err <= bound, (label, err, bound)


def check_summary(summary, ref, label):
    have = np.arange(ref.slots)[:, None] < np.minimum(ref.ep_count, ref.slots)[None, :]
    x, lengths = ref.ledger_return[have].tolist(), ref.ledger_length[have].tolist()
    assert summary[0] == len(x), label
    if not x:
        assert np.isnan(summary[1:]).all(), label
        return
    mean, std = R.exact_mean_std(x)
    assert abs(summary[1] - mean) <= R.mean_bound(x), (label, summary[1], mean, R.mean_bound(x))
    assert abs(summary[2] - std) <= R.std_bound(x), (label, summary[2], std, R.std_bound(x))
    assert abs(summary[3] - sum(lengths) / len(x)) <= 2 * R.U * sum(lengths) / len(x), label
    assert summary[4] == min(x) and summary[5] == max(x), label


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("K", STEPS)
@pytest.mark.parametrize("n", SIZES)
def test_three_calls_against_the_restatement(lib, n, K, pattern):
    """Three consecutive calls with the carry kept, in both input forms, a ledger of 3 slots (fewer than the episodes
    that complete under "all" and often under "bernoulli") pre-filled with NaN / -1 between guard rows."""
    rng = np.random.default_rng([n, K, PATTERNS.index(pattern)])
    ref = R.State(n, slots=3)
    by_dones, by_starts = Host(n, slots=3), Host(n, slots=3)
    for call in range(3):
        rewards, ends = make_rewards(K, n, rng), make_ends(pattern, K, n, rng)
        R.scan(ref, rewards, ends)
        assert by_dones.scan(lib, rewards, ends, "dones") == 0
        # row 0 of episode_starts is not read: give it noise
        assert by_starts.scan(lib, rewards, ends, "starts", first_row=rng.integers(0, 2, n).astype(np.uint8)) == 0
        for h, form in ((by_dones, "dones"), (by_starts, "starts")):
            label = (n, K, pattern, call, form)
            check_per_env(h, ref, label)
            check_totals(h.totals, ref.counted, label)  # the totals are a window over all calls so far
        assert same_bits(by_dones.totals, by_starts.totals)
    if pattern == "all":
        assert (ref.ep_count == 3 * K).all() and by_dones.totals[0] == 3 * K * n
    check_summary(by_dones.summary(lib), ref, (n, K, pattern))
    assert same_bits(by_dones.summary(lib), by_starts.summary(lib))


@pytest.mark.parametrize("slots", [0, 2, 4])
def test_targets_mixed_over_0_1_3(lib, slots):
    """evaluate_policy's rule: env i counts its first targets[i] episodes; later ones clear the carry and nothing else."""
    n, K = 65, 33
    rng = np.random.default_rng(slots)
    targets = rng.choice([0, 1, 3], n).astype(np.int32)
    assert set(targets.tolist()) == {0, 1, 3}
    ref, h = R.State(n, slots=slots, targets=targets), Host(n, slots=slots, targets=targets)
    for call in range(3):
        rewards, ends = make_rewards(K, n, rng), rng.random((K, n)) < 0.3
        R.scan(ref, rewards, ends)
        assert h.scan(lib, rewards, ends, "dones" if call != 1 else "starts") == 0
        check_per_env(h, ref, (slots, call))
        check_totals(h.totals, ref.counted, (slots, call))
    assert np.array_equal(h.ep_count, targets)  # 99 steps at p = 0.3: every env reached its target
    assert h.totals[0] == targets.sum()
    if slots:
        check_summary(h.summary(lib), ref, slots)


def test_sb3_counting_rule_matches_the_scan(lib):
    """The restated evaluate_policy loop over a recording and the scan with its targets agree on the episode multiset
    and, ordered by (end step, env), on the lists."""
    n, T, n_eval = 5, 60, 12
    rng = np.random.default_rng(3)
    rewards, dones = make_rewards(T, n, rng), rng.random((T, n)) < 0.25
    ep_r, ep_l = R.sb3_evaluate(rewards, dones, n_eval)
    targets = R.targets_for(n_eval, n)
    assert targets.tolist() == [2, 2, 2, 3, 3] and len(ep_r) == n_eval
    h = Host(n, slots=3, targets=targets)
    for k0 in range(0, T, 4):  # four steps per call
        assert h.scan(lib, rewards[k0:k0 + 4].copy(), dones[k0:k0 + 4], "dones") == 0
    assert h.totals[0] == n_eval
    have = np.arange(3)[:, None] < h.ep_count[None, :]
    ends = np.cumsum(np.where(have, h.ledger_length, 0), axis=0)
    slot, env = np.nonzero(have)
    at = np.lexsort((env, ends[slot, env]))
    assert h.ledger_return[slot[at], env[at]].tolist() == ep_r and h.ledger_length[slot[at], env[at]].tolist() == ep_l


def test_without_totals_and_without_ledger(lib):
    n, K = 63, 16
    rng = np.random.default_rng(1)
    rewards, ends = make_rewards(K, n, rng), rng.random((K, n)) < 0.2
    ref, h = R.State(n), Host(n, totals=False)
    R.scan(ref, rewards, ends)
    assert h.scan(lib, rewards, ends, "dones") == 0
    check_per_env(h, ref, "bare")


def test_totals_are_added_to_what_is_passed_in(lib):
    """min / max of a passed-in window count only when its episode count is positive."""
    rewards = np.array([[2.0], [3.0]], np.float32)
    ends = np.array([[True], [True]])
    h = Host(1)
    h.totals[:] = [0.0, 0.0, 0.0, -5.0, 50.0]  # an empty window: its min / max mean nothing
    assert h.scan(lib, rewards, ends, "dones") == 0
    assert h.totals.tolist() == [2.0, 5.0, 2.0, 2.0, 3.0]
    h.totals[:] = [4.0, 10.0, 7.0, 2.5, 2.75]
    assert h.scan(lib, rewards, ends, "dones") == 0
    assert h.totals.tolist() == [6.0, 15.0, 9.0, 2.0, 3.0]


def test_invalid_arguments_are_refused_and_write_nothing(lib):
    n, K = 4, 3
    rewards = np.ones((K, n), np.float32)
    d = np.ones((K, n), np.uint8)
    s, l = np.ones((K, n), np.uint8), np.ones(n, np.uint8)
    h = Host(n, slots=2)

    def call(k=K, nn=n, r=rewards, dones=None, starts=None, last=None, slots=2, lr=h.ledger_return, ll=h.ledger_length,
             rr=h.run_return, rl=h.run_length, cnt=h.ep_count):
        return lib.mse_episode_scan_host(k, nn, _p(r), _p(dones), _p(starts), _p(last), _p(rr), _p(rl), _p(cnt), None, slots,
                                         _p(lr), _p(ll), _p(h.totals))

    bad = [dict(dones=d, starts=s, last=l), dict(), dict(dones=d, last=l), dict(dones=d, starts=s), dict(starts=s), dict(last=l),
           dict(dones=d, k=0), dict(dones=d, k=-1), dict(dones=d, nn=0), dict(dones=d, nn=-3), dict(dones=d, r=None),
           dict(dones=d, rr=None), dict(dones=d, rl=None), dict(dones=d, cnt=None), dict(dones=d, lr=None), dict(dones=d, ll=None),
           dict(dones=d, slots=0), dict(dones=d, slots=-1), dict(dones=d, slots=2, lr=None, ll=None)]
    for kw in bad:
        assert call(**kw) == INVALID, kw
        assert b"mse_episode_scan_host" in lib.mse_last_error()
    assert not h.run_return.any() and not h.run_length.any() and not h.ep_count.any() and not h.totals.any()
    assert np.isnan(h.ledger_return).all() and (h.ledger_length == -1).all()
    assert call(dones=d) == 0 and call(starts=s, last=l) == 0  # the two legal forms
    # the device entry points check their arguments before any device call, so these hold without a device too
    ws = np.zeros(int(lib.mse_episode_workspace_bytes()), np.uint8)
    for kw in (dict(dones=d, starts=s, last=l), dict(), dict(dones=d, k=0), dict(dones=d, nn=0)):
        rc = lib.mse_episode_scan(kw.get("k", K), kw.get("nn", n), _p(rewards), _p(kw.get("dones")), _p(kw.get("starts")),
                                  _p(kw.get("last")), _p(h.run_return), _p(h.run_length), _p(h.ep_count), None, 0, None, None,
                                  _p(h.totals), _p(ws), None)
        assert rc == INVALID and b"mse_episode_scan:" in lib.mse_last_error(), kw


def test_a_summary_needs_a_ledger(lib):
    cnt, out = np.zeros(4, np.int32), np.full(6, -7.0)
    lr, ll = np.zeros((2, 4)), np.zeros((2, 4), np.int32)
    for fn, tail in ((lib.mse_episode_summary_host, ()), (lib.mse_episode_summary, (None,))):
        assert fn(4, 0, _p(cnt), None, None, _p(out), *tail) == INVALID
        assert fn(4, 2, _p(cnt), None, _p(ll), _p(out), *tail) == INVALID
        assert fn(4, 2, _p(cnt), _p(lr), None, _p(out), *tail) == INVALID
        assert fn(4, 0, _p(cnt), _p(lr), _p(ll), _p(out), *tail) == INVALID
        assert fn(0, 2, _p(cnt), _p(lr), _p(ll), _p(out), *tail) == INVALID
        assert b"mse_episode_summary" in lib.mse_last_error()
    assert out.tolist() == [-7.0] * 6
    assert lib.mse_episode_workspace_bytes() >= 5 * 8 and lib.mse_episode_workspace_bytes() % 8 == 0


def test_summary_of_known_values(lib):
    """[1, 2, 3, 4] -> mean 2.5, population std sqrt(1.25); a count past the slots is clipped to the ledger."""
    cnt = np.array([2, 5], np.int32)
    lr = np.array([[1.0, 3.0], [2.0, 4.0]])
    ll = np.array([[10, 30], [20, 40]], np.int32)
    out = np.zeros(6)
    assert lib.mse_episode_summary_host(2, 2, _p(cnt), _p(lr), _p(ll), _p(out)) == 0
    assert out.tolist() == [4.0, 2.5, math.sqrt(1.25), 25.0, 1.0, 4.0]
