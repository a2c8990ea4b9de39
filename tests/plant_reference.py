"""numpy restatement of the plant ledger (include/mse.h "Plant ledger"), written from the reference's definitions and not
from the C code: it goes from LEDGER LISTS - the bale tuples (size, stored quality) per material, the press log's codes, the
(r_sort, r_press) pairs and the step rewards of ONE episode - straight to the row of 32 columns.

    row_from_ledgers()   one episode's lists -> the row
    Ledgers              the lists themselves, built record by record with the reference's list-form press_bale
                         (src/envs_train/env_super.py:661-687): what a run of the reference would have appended
    rows_from_records()  the records of one env, [T, 40] -> the rows of its closed episodes and the open episode's Ledgers
    scan()               one call of mse_plant_scan_host on a State (open Ledgers per env, counts, ledger, totals)
    avg_bale_deviation() np.mean of |size - S| / S over all bales (env_super.py:235-241)

Bales stay lists here; the code under test keeps O(1) sums.  A return is a sequential float64 sum in step order."""
import numpy as np

COLS, RUN_COLS = 32, 36
MATERIALS = "ABCDE"
# record columns (include/mse.h MSE_TRACE_*)
R_SORT, R_PRESS, CONT_TRUE, CONT_FALSE, CONT_E, N_LOG, LOG, N_BALE, BALE, DONE, REWARD, OVERFLOW = 1, 2, 8, 12, 16, 17, 18, 22, 23, 29, 32, 37


def seq_sum(values):
    """the float64 sum in order: 0.0 + v0 + v1 + ..."""
    s = np.float64(0.0)
    for v in values:
        s = s + np.float64(v)
    return float(s)


def row_from_ledgers(rewards, reward_pairs, press_codes, bales, S, overflow, left_over):
    """rewards: the step rewards; reward_pairs: [(r_sort, r_press)]; press_codes: the press log's codes in order;
    bales: {material: [(size, q)]}; overflow / left_over: the closing step's."""
    row = np.zeros(COLS, np.float64)
    row[0] = len(rewards)
    row[1] = seq_sum(rewards)
    row[2] = seq_sum(p[0] for p in reward_pairs)
    row[3] = seq_sum(p[1] for p in reward_pairs)
    codes = [int(c) for c in press_codes]
    row[4], row[5] = codes.count(1), codes.count(2)
    row[6] = codes.count(111) + codes.count(222)
    row[7] = codes.count(0)
    row[8], row[9] = overflow, left_over
    for m, name in enumerate(MATERIALS):
        lst = [(int(size), int(q)) for size, q in bales[name]]
        row[10 + m] = len(lst)
        row[15 + m] = sum(size for size, _ in lst)
        row[20 + m] = sum(q for _, q in lst)
        row[25 + m] = sum(abs(size - S) for size, _ in lst)
    return row


def avg_bale_deviation(bales, S):
    dev = [abs(size - S) / S for name in MATERIALS for size, _ in bales[name]]
    return float(np.mean(dev)) if dev else 0.0


class Ledgers:
    """The lists of one open episode."""

    def __init__(self, S, remainder_units):
        self.S, self.U = int(S), int(remainder_units)
        self.clear()

    def clear(self):
        self.rewards, self.pairs, self.codes = [], [], []
        self.bales = {m: [] for m in MATERIALS}

    def press_bale(self, material, n, q):
        bales, S = self.bales[material], self.S
        for _ in range(n // S):
            bales.append((S, q))
        rem = n % S
        if rem > 0:
            if rem > self.U:  # rem > S * threshold, on integers
                bales.append((rem, q))
            elif bales:
                bales[-1] = (bales[-1][0] + rem, bales[-1][1])
            else:
                bales.append((rem, q))

    def append(self, rec):
        """One record; returns the episode's row if the record closes it (the lists are then cleared), else None."""
        for b in range(int(rec[N_BALE])):
            m, n, q = (int(rec[BALE + 3 * b + c]) for c in range(3))
            self.press_bale(MATERIALS[m], n, q)
        for j in range(int(rec[N_LOG])):
            self.codes.append(int(rec[LOG + 2 * j]))
        self.rewards.append(rec[REWARD])
        self.pairs.append((rec[R_SORT], rec[R_PRESS]))
        if rec[DONE] == 0:
            return None
        left = rec[CONT_TRUE:CONT_TRUE + 4].sum() + rec[CONT_FALSE:CONT_FALSE + 4].sum() + rec[CONT_E]
        row = row_from_ledgers(self.rewards, self.pairs, self.codes, self.bales, self.S, rec[OVERFLOW], left)
        self.clear()
        return row

    def carry(self):
        """What the run[] column of this env must hold: the open episode's columns 0-29 (8, 9 zero), the last bale sizes,
        and a last row the scan does not touch (returned as 0)."""
        row = row_from_ledgers(self.rewards, self.pairs, self.codes, self.bales, self.S, 0.0, 0.0)
        out = np.zeros(RUN_COLS, np.float64)
        out[:30] = row[:30]
        for m, name in enumerate(MATERIALS):
            out[30 + m] = self.bales[name][-1][0] if self.bales[name] else 0
        return out


def rows_from_records(records, S, remainder_units):
    """records [T, 40] of one env -> ([row per closed episode], the open episode's Ledgers)"""
    led, rows = Ledgers(S, remainder_units), []
    for rec in np.asarray(records, np.float64):
        row = led.append(rec)
        if row is not None:
            rows.append(row)
    return rows, led


class State:
    def __init__(self, n, S, remainder_units, slots=0, targets=None):
        self.n, self.slots = n, slots
        self.open = [Ledgers(S, remainder_units) for _ in range(n)]
        self.ep_count = np.zeros(n, np.int32)
        self.targets = None if targets is None else np.asarray(targets, np.int32)
        self.ledger = np.full((slots, COLS, n), np.nan, np.float64) if slots else None
        self.counted = []  # (env, row) of every counted episode, those beyond the slots included, in (env, step) order

    def run(self):
        return np.stack([l.carry() for l in self.open], axis=1)


def scan(state, records):
    """records f64[K, 40, N]; the counted episodes go to state.ledger / state.counted"""
    K, _, n = records.shape
    for i in range(n):
        for k in range(K):
            row = state.open[i].append(records[k, :, i])
            if row is None:
                continue
            c = int(state.ep_count[i])
            if state.targets is None or c < state.targets[i]:
                if state.ledger is not None and c < state.slots:
                    state.ledger[c, :, i] = row
                state.counted.append((i, row))
                state.ep_count[i] = c + 1


def totals_of(counted):
    """f64[33] from the counted episodes: the integer cells exactly, cells 1-3 with math.fsum"""
    import math

    t = np.zeros(1 + COLS, np.float64)
    t[0] = len(counted)
    for c in range(COLS):
        col = [float(row[c] != 0) if c == 8 else float(row[c]) for _, row in counted]
        t[1 + c] = math.fsum(col)
    return t


def random_records(rng, K, n, S, p_done=0.1):
    """Synthetic but well-formed records f64[K, 40, n]: every branch of the press_bale rule, all five codes, rewards of
    mixed sign and magnitude, episode ends with probability p_done."""
    rec = np.zeros((K, 40, n), np.float64)
    rec[:, REWARD] = rng.standard_normal((K, n)) * 10.0 ** rng.integers(-3, 2, (K, n))
    rec[:, R_SORT] = rng.standard_normal((K, n))
    rec[:, R_PRESS] = rec[:, REWARD] - rec[:, R_SORT]
    rec[:, CONT_TRUE:CONT_TRUE + 4] = rng.integers(0, 300, (K, 4, n))
    rec[:, CONT_FALSE:CONT_FALSE + 4] = rng.integers(0, 60, (K, 4, n))
    rec[:, CONT_E] = rng.integers(0, 300, (K, n))
    rec[:, N_LOG] = rng.integers(0, 3, (K, n))
    rec[:, N_BALE] = rng.integers(0, 3, (K, n))
    for j in range(2):
        rec[:, LOG + 2 * j] = rng.choice([0, 1, 2, 111, 222], (K, n))
        rec[:, LOG + 2 * j + 1] = rng.integers(-1, 5, (K, n))
        rec[:, BALE + 3 * j] = rng.integers(0, 5, (K, n))
        rec[:, BALE + 3 * j + 1] = rng.integers(0, 3 * S + 1, (K, n)) * (rng.random((K, n)) < 0.9)
        rec[:, BALE + 3 * j + 2] = rng.integers(0, 101, (K, n))
    rec[:, DONE] = rng.random((K, n)) < p_done
    rec[:, OVERFLOW] = rec[:, DONE] * rng.integers(0, 6, (K, n)) * (rng.random((K, n)) < 0.5)
    return rec
