"""CPU checks of the plant ledger (no device needed): `mse_plant_scan_host`, which runs the inline functions of
marl-sortingenv_amd/csrc/mse_plant_math.h that the kernel runs, against tests/plant_reference.py (numpy, from ledger LISTS
to the row by the reference's definitions).  Integer columns are exact.  Columns 1-3 against the FIXTURES' float64 ledgers
are held within T x 1e-12, the oracle's own reward bound over T steps; against plant_reference on the SAME records they
are the same additions in the same order, so bit-equal."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import marl_sortingenv_amd as M
from marl_sortingenv_amd.config import SortingEnvConfig
from marl_sortingenv_amd.trace import EnvTrace
from oracle.oracle import OracleEnv, STEP_CHECK_OVERFLOW, STEP_UNMASKED
from tests import plant_reference as R
from tests import replay

INVALID, ALIGNMENT = -1, -6
INT_COLS = [0] + list(range(4, 32))
SUM_COLS = [1, 2, 3]
TRACE_FIXTURES = sorted(glob.glob(os.path.join(replay.GOLDEN_DIR, "trace_*.npz")))


@pytest.fixture(scope="module")
def lib():
    return M.load_library()


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


class Host:
    """Caller-owned arrays of one accounting; run and the ledger lie between guard rows, totals between guard cells."""

    def __init__(self, n, S, U, slots=0, targets=None, totals=True):
        self.n, self.S, self.U, self.slots = n, S, U, slots
        self._run = np.zeros((R.RUN_COLS + 2, n), np.float64)
        self._run[[0, -1]] = np.nan
        self.run = self._run[1:-1]
        self.ep_count = np.zeros(n, np.int32)
        self.targets = None if targets is None else np.ascontiguousarray(targets, np.int32)
        self._led = np.full((slots * R.COLS + 2, n), np.nan, np.float64)
        self.ledger = self._led[1:-1].reshape(slots, R.COLS, n) if slots else None
        self._tot = np.zeros(1 + R.COLS + 2, np.float64)
        self._tot[[0, -1]] = np.nan
        self.totals = self._tot[1:-1] if totals else None

    def scan(self, lib, records):
        records = np.ascontiguousarray(records, np.float64)
        return lib.mse_plant_scan_host(records.shape[0], self.n, _p(records), self.S, self.U, _p(self.run), _p(self.ep_count),
                                       _p(self.targets), self.slots, _p(self.ledger), _p(self.totals))

    def guards_intact(self):
        return bool(np.isnan(self._run[[0, -1]]).all() and np.isnan(self._led[[0, -1]]).all() and np.isnan(self._tot[[0, -1]]).all())


def fixture_records(path):
    """The fixture's rows replayed through the oracle: (meta, z, records [T, 40])."""
    meta, z = replay.load(path)
    env = OracleEnv(kind=meta["kind"], max_steps=meta["max_steps"], seed=meta["ctor_seed"], noise_sorting=meta["noise_sorting"],
                    balesize=meta["balesize"])
    recs = []
    for t in range(len(z["op"])):
        if z["op"][t] == 1:
            env.reset(int(z["arg"][t]))
            assert not recs, "the trace fixtures hold one episode"
        else:
            f = int(z["flags"][t])
            env.step(int(z["arg"][t]), int(z["sort_mode"][t]), use_action_masking=not (f & STEP_UNMASKED),
                     check_overflow=bool(f & STEP_CHECK_OVERFLOW))
            recs.append(env.trace_record())
    return meta, z, np.asarray(recs)


def fixture_row(meta, z):
    """plant_reference on the fixture's ledger_* arrays (the lists the reference itself appended)."""
    cfg = SortingEnvConfig()
    S = int(meta["balesize"])
    steps = z["op"] != 1
    true, false = z["ledger_true"][-1], z["ledger_false"][-1]
    levels = [int(true[m] + false[m]) for m in range(5)]
    overflow = 0
    if (int(z["flags"][-1]) & STEP_CHECK_OVERFLOW) and bool(z["terminated"][-1]):
        over = [m for m in range(5) if levels[m] > cfg.container_capacity]
        overflow = over[0] + 1 if over else 0
    bales = {m: [tuple(b) for b in z["ledger_bales_" + m].tolist()] for m in R.MATERIALS}
    row = R.row_from_ledgers(z["reward"][steps], z["ledger_reward"], z["ledger_press_log"][:, 0], bales, S, overflow, sum(levels))
    return row, bales


def test_fixtures_against_the_reference_ledgers(lib):
    seen = set()
    for path in TRACE_FIXTURES:
        meta, z, recs = fixture_records(path)
        S = int(meta["balesize"])
        U = int(np.floor(S * 0.5))
        T = len(recs)
        assert bool(z["terminated"][-1]) and recs[-1, R.DONE] != 0, "one closed episode per fixture"
        h = Host(1, S, U, slots=2)
        assert h.scan(lib, recs[:, :, None]) == 0
        exp, bales = fixture_row(meta, z)
        got = h.ledger[0, :, 0]
        label = meta["name"]
        assert h.ep_count[0] == 1 and h.totals[0] == 1.0, label
        assert np.array_equal(got[INT_COLS], exp[INT_COLS]), (label, got, exp)
        assert np.all(np.abs(got[SUM_COLS] - exp[SUM_COLS]) <= T * 1e-12), (label, got[SUM_COLS], exp[SUM_COLS])
        assert np.all(h.run[:R.RUN_COLS - 1] == 0.0), label  # the carry is cleared at the episode's end
        assert np.isnan(h.ledger[1]).all() and h.guards_intact(), label
        # the reference's average bale deviation, formed once outside the sums
        n_bales = got[10:15].sum()
        if n_bales:
            assert abs(got[25:30].sum() / (S * n_bales) - R.avg_bale_deviation(bales, S)) <= 1e-12, label
        # the package's own list form (EnvTrace) agrees with the fixture's lists, so from_records is held too
        tr = EnvTrace.from_records(recs[:, :, None], 0, S, 0.5)
        assert {m: [tuple(b) for b in tr.bale_count[m]] for m in R.MATERIALS} == bales, label
        # branch coverage over the set
        sizes = [size for m in R.MATERIALS for size, _ in bales[m]]
        seen |= {"merged"} if any(s > S for s in sizes) else set()
        seen |= {"short"} if any(s < S for s in sizes) else set()
        seen |= {"full"} if any(s == S for s in sizes) else set()
        codes = set(z["ledger_press_log"][:, 0].tolist())
        seen |= {f"code{c}" for c in codes}
        seen |= {"noop_only"} if codes == {0} else set()
        seen |= {"overflow"} if exp[8] != 0 else set()
        if exp[8] != 0:
            assert T == 20 and label == "trace_mono_n5_overflow_s1"
    assert len(TRACE_FIXTURES) == 6
    assert seen >= {"merged", "short", "full", "code0", "code1", "code2", "code111", "code222", "noop_only", "overflow"}, seen


def record(bales=(), codes=(), reward=0.0, r_sort=0.0, r_press=0.0, done=0, overflow=0, cont=0):
    rec = np.zeros(40, np.float64)
    rec[R.N_BALE] = len(bales)
    for b, (m, n, q) in enumerate(bales):
        rec[R.BALE + 3 * b:R.BALE + 3 * b + 3] = (m, n, q)
    rec[R.N_LOG] = len(codes)
    for j, c in enumerate(codes):
        rec[R.LOG + 2 * j] = c
    rec[R.REWARD], rec[R.R_SORT], rec[R.R_PRESS], rec[R.DONE], rec[R.OVERFLOW], rec[R.CONT_E] = reward, r_sort, r_press, done, overflow, cont
    return rec


def scan_one(lib, recs, S=200, U=100):
    h = Host(1, S, U, slots=4)
    assert h.scan(lib, np.asarray(recs)[:, :, None]) == 0
    rows, open_ = R.rows_from_records(recs, S, U)
    assert h.ep_count[0] == len(rows)
    for e, row in enumerate(rows):
        assert same_bits(h.ledger[e, :, 0], row), (e, h.ledger[e, :, 0], row)
    assert same_bits(h.run[:R.RUN_COLS - 1, 0], open_.carry()[:R.RUN_COLS - 1])
    assert h.guards_intact()
    return h


def test_synthetic_records(lib):
    S, U = 200, 100
    # a small remainder with no earlier bale opens one; n = 0 changes nothing
    h = scan_one(lib, [record(bales=[(2, 40, 77)]), record(bales=[(1, 0, 50)], done=1)])
    row = h.ledger[0, :, 0]
    assert row[10 + 2] == 1 and row[15 + 2] == 40 and row[20 + 2] == 77 and row[25 + 2] == 160
    assert row[10 + 1] == 0 and row[15 + 1] == 0 and row[20 + 1] == 0 and row[25 + 1] == 0
    # two press_bale calls of one material in one step: 450 -> 200, 200 and 50 merged into the second; then 30 merged again
    h = scan_one(lib, [record(bales=[(0, 450, 90), (0, 30, 10)], done=1)])
    row = h.ledger[0, :, 0]
    assert row[10] == 2 and row[15] == 480 and row[20] == 180 and row[25] == 80
    # a remainder of exactly remainder_units merges, remainder_units + 1 opens a bale
    h = scan_one(lib, [record(bales=[(3, S, 80)]), record(bales=[(3, U, 60)]), record(bales=[(3, U + 1, 70)], done=1)])
    row = h.ledger[0, :, 0]
    assert row[10 + 3] == 2 and row[15 + 3] == S + U + U + 1 and row[20 + 3] == 150 and row[25 + 3] == U + (S - U - 1)
    # exactly remainder_units with no earlier bale opens one (there is nothing to merge into)
    h = scan_one(lib, [record(bales=[(4, U, 0)], done=1)])
    assert h.ledger[0, 10 + 4, 0] == 1 and h.ledger[0, 25 + 4, 0] == S - U
    # a merge onto a short bale can shrink the deviation; the last size survives a call boundary (carry rows 30-34)
    h = scan_one(lib, [record(bales=[(1, 150, 55)]), record(bales=[(1, 30, 99)])])
    assert h.run[10 + 1, 0] == 1 and h.run[25 + 1, 0] == 20 and h.run[30 + 1, 0] == 180 and h.run[20 + 1, 0] == 55
    # the press codes, the closing step's overflow and containers, the three sums
    h = scan_one(lib, [record(codes=[1, 222], reward=0.1, r_sort=0.3, r_press=-0.2), record(codes=[111]),
                       record(codes=[0, 2], reward=0.2, r_sort=0.1, r_press=0.1, done=1, overflow=3, cont=17)])
    row = h.ledger[0, :, 0]
    assert row[[0, 4, 5, 6, 7, 8, 9]].tolist() == [3, 1, 1, 2, 1, 3, 17] and h.totals[1 + 8] == 1.0
    assert row[1] == (0.0 + 0.1) + 0.0 + 0.2 and row[30] == 0 and row[31] == 0


def oracle_records(n_envs, K, seed):
    """Several oracle envs with short episodes (max_steps 12-30) stepped with random actions: records f64[K, 40, n]."""
    rng = np.random.default_rng(seed)
    rec = np.zeros((K, 40, n_envs), np.float64)
    for i in range(n_envs):
        kind = ("mono", "press", "sort")[i % 3]
        env = OracleEnv(kind=kind, max_steps=12 + (7 * i) % 19, seed=100 + i, noise_sorting=0.05 * (i % 2))
        env.reset(100 + i)
        for k in range(K):
            legal = np.flatnonzero(env.action_masks())
            env.step(int(rng.choice(legal)), check_overflow=True)
            rec[k, :, i] = env.trace_record()
            if rec[k, R.DONE, i] != 0:
                env.reset()
    return rec


@pytest.fixture(scope="module")
def multi():
    return oracle_records(7, 90, seed=5)


def check_against_reference(h, st, totals_before=None):
    assert np.array_equal(h.ep_count, st.ep_count)
    assert same_bits(h.run[:R.RUN_COLS - 1], st.run()[:R.RUN_COLS - 1])
    if h.slots:
        assert np.array_equal(np.isnan(h.ledger), np.isnan(st.ledger))  # cells of episodes that did not happen are not written
        assert same_bits(np.nan_to_num(h.ledger), np.nan_to_num(st.ledger))
    if h.totals is not None:
        exp = R.totals_of(st.counted) + (0 if totals_before is None else totals_before)
        ints = [0] + [1 + c for c in INT_COLS]
        assert np.array_equal(h.totals[ints], exp[ints])
        for c in SUM_COLS:  # a sum of `terms` doubles in any order: within terms x 2^-52 x sum |x|
            terms = len(st.counted) + 1
            mag = sum(abs(row[c]) for _, row in st.counted) + (0 if totals_before is None else abs(totals_before[1 + c]))
            assert abs(h.totals[1 + c] - exp[1 + c]) <= terms * 2.0 ** -52 * mag
    assert h.guards_intact()


def test_multi_episode_splits_targets_slots_totals(lib, multi):
    K, _, n = multi.shape
    S, U = 200, 100
    ends = (multi[:, R.DONE] != 0).sum(axis=0)
    assert ends.min() >= 3 and (multi[K - 1, R.DONE] == 0).any(), "episodes must end mid-buffer and stay open at its end"
    whole = Host(n, S, U, slots=3)
    assert whole.scan(lib, multi) == 0
    st = R.State(n, S, U, slots=3)
    R.scan(st, multi)
    check_against_reference(whole, st)
    assert (whole.ep_count > 3).any(), "episodes beyond the slots are counted but not stored"
    # every split K1 + K2 gives the same bits: the carry
    for k1 in range(1, K):
        h = Host(n, S, U, slots=3)
        assert h.scan(lib, multi[:k1]) == 0 and h.scan(lib, multi[k1:]) == 0
        assert same_bits(h.run, whole.run) and same_bits(np.nan_to_num(h.ledger), np.nan_to_num(whole.ledger))
        assert np.array_equal(h.ep_count, whole.ep_count) and np.array_equal(h.totals[[0] + [1 + c for c in INT_COLS]],
                                                                             whole.totals[[0] + [1 + c for c in INT_COLS]])
        assert np.all(np.abs(h.totals[1:4] - whole.totals[1:4]) <= 2.0 ** -40)
    # the targets rule (0: none counted; 2: the first two), with and without room in the ledger
    targets = np.array([0, 1, 2, 5, 2, 1, 100], np.int32)
    for slots in (0, 1, 4):
        h = Host(n, S, U, slots=slots, targets=targets)
        assert h.scan(lib, multi) == 0
        st = R.State(n, S, U, slots=slots, targets=targets)
        R.scan(st, multi)
        check_against_reference(h, st)
        assert np.array_equal(h.ep_count, np.minimum(targets, ends))
    # totals are added onto what is passed in; totals = NULL
    before = np.arange(1 + R.COLS, dtype=np.float64) * 0.5
    h = Host(n, S, U, slots=3)
    h.totals[:] = before
    assert h.scan(lib, multi) == 0
    st = R.State(n, S, U, slots=3)
    R.scan(st, multi)
    check_against_reference(h, st, totals_before=before)
    h = Host(n, S, U, slots=3, totals=False)
    assert h.scan(lib, multi) == 0
    check_against_reference(h, st)


def test_random_records_against_the_lists(lib):
    """Synthetic records hit every branch at once, at sizes around a wave and the 256-lane group."""
    rng = np.random.default_rng(11)
    for n, K, S, U in ((1, 33, 200, 100), (65, 16, 150, 75), (257, 7, 7, 0), (64, 5, 1, 0)):
        rec = R.random_records(rng, K, n, S)
        h = Host(n, S, U, slots=2)
        assert h.scan(lib, rec) == 0
        st = R.State(n, S, U, slots=2)
        R.scan(st, rec)
        check_against_reference(h, st)


def test_refusals_in_order_and_nothing_written(lib):
    S, U, n, K = 200, 100, 3, 4
    rec = R.random_records(np.random.default_rng(2), K, n, S, p_done=0.5)
    odd = np.zeros(8 * (K * 40 * n + 1), np.uint8)[4:4 + 8 * K * 40 * n]  # a 4-byte-aligned address that is not 8-byte aligned
    assert odd.ctypes.data % 8 == 4

    def call(host_form, h, k=K, nn=n, records=rec, s=S, u=U, run=True, ep=True, slots=None, ledger=True, totals=True, workspace=None):
        args = [k, nn, _p(records), s, u, _p(h.run) if run else None, _p(h.ep_count) if ep else None, None,
                h.slots if slots is None else slots, (_p(h.ledger) if ledger else None), (_p(h.totals) if totals else None)]
        if host_form:
            return lib.mse_plant_scan_host(*args)
        return lib.mse_plant_scan(*args, workspace, None)

    for host_form in (True, False):
        name = "mse_plant_scan_host" if host_form else "mse_plant_scan"
        h = Host(n, S, U, slots=2)
        h.ep_count[:] = 7
        cases = [
            # each case breaks one rule and every LATER rule too: the earliest one must be the one reported
            (dict(k=0, records=None, slots=-1, s=0), INVALID, "k_steps and n must be positive"),
            (dict(nn=0, records=None, slots=-1, s=0), INVALID, "k_steps and n must be positive"),
            (dict(records=None, slots=-1, s=0), INVALID, "records, run and ep_count must be given"),
            (dict(run=False, slots=-1, s=0), INVALID, "records, run and ep_count must be given"),
            (dict(ep=False, slots=-1, s=0), INVALID, "records, run and ep_count must be given"),
            (dict(slots=-1, s=0), INVALID, "slots must be positive with a ledger and 0 without"),
            (dict(slots=0, s=0), INVALID, "slots must be positive with a ledger and 0 without"),
            (dict(ledger=False, s=0), INVALID, "slots must be positive with a ledger and 0 without"),
            (dict(s=0, records=odd), INVALID, "bale_standard_size must be positive"),
            (dict(u=-1, records=odd), INVALID, "bale_standard_size must be positive"),
            (dict(u=S, records=odd), INVALID, "bale_standard_size must be positive"),
            (dict(records=odd), ALIGNMENT, "8-byte aligned"),
        ]
        if not host_form:
            # totals without a workspace: after the value rules, before alignment
            cases.insert(len(cases) - 1, (dict(records=odd, workspace=None), INVALID, "totals need a workspace"))
            cases[-1] = (dict(records=odd, workspace=_p(h._tot)), ALIGNMENT, "8-byte aligned")
        for kw, status, text in cases:
            assert call(host_form, h, **kw) == status, (name, kw)
            msg = lib.mse_last_error().decode()
            assert msg.startswith(name + ":") and text in msg, (name, kw, msg)
            assert np.all(h.run == 0) and np.all(h.ep_count == 7) and np.isnan(h.ledger).all() and np.all(h.totals == 0) and h.guards_intact()


def test_from_records_splits_episodes(multi):
    i = 3
    rows = multi[:, :, i]
    ends = np.flatnonzero(rows[:, R.DONE] != 0)
    tr = EnvTrace.from_records(multi, i, episode=1)
    assert len(tr.records) == ends[1] - ends[0] and np.array_equal(tr.records[0], rows[ends[0] + 1])
    led = R.Ledgers(200, 100)
    segment = rows[ends[0] + 1:ends[1] + 1].copy()
    segment[-1, R.DONE] = 0  # keep the lists: a closing record clears them
    for r in segment:
        led.append(r)
    assert {m: list(tr.bale_count[m]) for m in R.MATERIALS} == led.bales
    assert len(EnvTrace.from_records(multi, i).records) == len(rows)
    with pytest.raises(IndexError):
        EnvTrace.from_records(multi, i, episode=len(ends) + 1)
    with pytest.raises(ValueError):
        EnvTrace.from_records(multi, multi.shape[2])
