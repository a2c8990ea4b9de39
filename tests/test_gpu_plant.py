"""GPU: the plant ledger kernel (mse_plant_scan) against its host twin on synthetic records at every launch shape - per-env
carry, ledger and counts bit for bit (columns 1-3 included: the same additions in the same order), the integer totals
exactly, totals 1-3 within terms x 2^-52 x sum |x|, a rerun bit-equal - and `evaluate_plant` against the reference's
rule-based benchmark figures and against `evaluate_policy`."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import plant_reference as R
from tests import replay
from tests.test_plant_cpu import INT_COLS, SUM_COLS, Host, same_bits

pytestmark = pytest.mark.gpu

BAND, SENTINEL = 64, -12345.0


def _grid_cap():
    import torch

    return min(torch.cuda.get_device_properties(0).multi_processor_count, 1024)  # workgroups of k_plant_scan at most


class Device:
    """The arrays of one accounting on the device, each between two sentinel bands"""

    def __init__(self, n, S, U, slots, targets=None):
        import torch

        import marl_sortingenv_amd as M

        self.n, self.S, self.U, self.slots = n, S, U, slots
        self.raw = []

        def banded(count, dtype):
            buf = torch.full((count + 2 * BAND,), SENTINEL, dtype=dtype, device="cuda")
            self.raw.append((buf, count))
            return buf[BAND:BAND + count]

        self.run = banded(R.RUN_COLS * n, torch.float64).view(R.RUN_COLS, n)
        self.ep_count = banded(n, torch.int32)
        self.ledger = banded(slots * R.COLS * n, torch.float64).view(slots, R.COLS, n) if slots else None
        self.totals = banded(1 + R.COLS, torch.float64)
        for t in (self.run, self.ep_count, self.totals):
            t.zero_()
        if slots:
            self.ledger.fill_(float("nan"))
        self.targets = None if targets is None else torch.as_tensor(targets, dtype=torch.int32, device="cuda")
        self.L = M.load_library()
        self.workspace = torch.empty(int(self.L.mse_plant_workspace_bytes()), dtype=torch.uint8, device="cuda")

    def scan(self, records, totals=True):
        import torch

        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        rec = torch.from_numpy(np.ascontiguousarray(records, np.float64)).cuda()
        torch.cuda.synchronize()
        rc = self.L.mse_plant_scan(records.shape[0], self.n, p(rec), self.S, self.U, p(self.run), p(self.ep_count), p(self.targets),
                                   self.slots, p(self.ledger), p(self.totals) if totals else None, p(self.workspace),
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, self.L.mse_last_error()
        torch.cuda.synchronize()

    def bands_intact(self):
        return all(bool((buf[:BAND] == SENTINEL).all()) and bool((buf[BAND + count:] == SENTINEL).all()) for buf, count in self.raw)


def compare(dev, host, terms, label):
    assert np.array_equal(dev.ep_count.cpu().numpy(), host.ep_count), label
    assert same_bits(dev.run[:R.RUN_COLS - 1].cpu().numpy(), host.run[:R.RUN_COLS - 1]), label
    assert bool((dev.run[R.RUN_COLS - 1] == 0).all()), label  # the last carry row is not touched
    if dev.slots:
        got, want = dev.ledger.cpu().numpy(), host.ledger
        assert np.array_equal(np.isnan(got), np.isnan(want)) and same_bits(np.nan_to_num(got), np.nan_to_num(want)), label
    got, want = dev.totals.cpu().numpy(), host.totals
    ints = [0] + [1 + c for c in INT_COLS]
    assert np.array_equal(got[ints], want[ints]), (label, got, want)
    for c in SUM_COLS:
        # both are sums of the same `terms` episode values in different orders: each within terms x 2^-53 x sum |x| of the
        # exact sum, so within terms x 2^-52 x sum |x| of each other
        assert abs(got[1 + c] - want[1 + c]) <= terms[0] * 2.0 ** -52 * terms[1 + SUM_COLS.index(c)], (label, c, got[1 + c], want[1 + c])
    assert dev.bands_intact() and host.guards_intact(), label


def sum_terms(host):
    """(number of counted episodes + 1, sum |x| of columns 1..3 over them), from the host ledger of a run with room for all"""
    led, cnt = host.ledger, host.ep_count
    have = np.arange(host.slots)[:, None] < cnt[None, :]
    assert cnt.max() <= host.slots
    return (int(have.sum()) + 1,) + tuple(float(np.abs(led[:, c, :][have]).sum()) for c in SUM_COLS)


PAST_THE_GRID = "one group past a full grid"
SHAPES = [(n, K) for n in (1, 64, 65, 256, 257) for K in (1, 7)] + [(PAST_THE_GRID, 1)]


@pytest.mark.parametrize("n,K", SHAPES, ids=lambda v: str(v).replace(" ", "_"))
def test_scan_against_the_host_twin(n, K):
    if n == PAST_THE_GRID:
        n = 256 * _grid_cap() + 257  # the grid-stride loop takes a second block, the last one partly filled
    S, U = (200, 100) if n % 2 else (150, 75)
    rng = np.random.default_rng(7 * n + K)
    slots = 2 * K + 1
    rec = [R.random_records(rng, K, n, S, p_done=0.3) for _ in range(2)]
    host, dev = Host(n, S, U, slots=slots), Device(n, S, U, slots)
    again = Device(n, S, U, slots)
    for r in rec:  # two calls: the carry crosses a call boundary on the device as on the host
        assert host.scan(dev.L, r) == 0
        dev.scan(r)
        again.scan(r)
    compare(dev, host, sum_terms(host), f"n={n} K={K}")
    # a rerun is bit-equal, totals 1-3 included: no atomics, a fixed reduction order
    assert same_bits(again.totals.cpu().numpy(), dev.totals.cpu().numpy())
    assert same_bits(again.run.cpu().numpy(), dev.run.cpu().numpy())


def test_scan_targets_small_ledger_and_no_totals():
    n, K, S, U = 257, 7, 200, 100
    rng = np.random.default_rng(3)
    rec = R.random_records(rng, K, n, S, p_done=0.5)
    targets = rng.integers(0, 4, n).astype(np.int32)
    import marl_sortingenv_amd as M

    full = Host(n, S, U, slots=K, targets=targets)
    assert full.scan(M.load_library(), rec) == 0
    terms = sum_terms(full)
    for slots in (0, 1):
        host, dev = Host(n, S, U, slots=slots, targets=targets), Device(n, S, U, slots, targets=targets)
        assert host.scan(dev.L, rec) == 0
        dev.scan(rec)
        compare(dev, host, terms, f"targets, slots={slots}")
        assert int(dev.totals[0]) == int(np.minimum(targets, (rec[:, R.DONE] != 0).sum(0)).sum())
    # totals = NULL: the per-env outputs are the same and totals stay as they were
    host, dev = Host(n, S, U, slots=2), Device(n, S, U, 2)
    dev.totals.fill_(5.0)
    assert host.scan(dev.L, rec) == 0
    dev.scan(rec, totals=False)
    assert bool((dev.totals == 5.0).all())
    assert same_bits(dev.run[:35].cpu().numpy(), host.run[:35]) and np.array_equal(dev.ep_count.cpu().numpy(), host.ep_count)
    assert same_bits(np.nan_to_num(dev.ledger.cpu().numpy()), np.nan_to_num(host.ledger)) and dev.bands_intact()


def test_evaluate_plant_rule_based_benchmark():
    """The reference's rule-based run for the paper's benchmark seeds 1..10, max_steps 200, noise 0: cumulative reward
    44.18 +- 1.38, held as tests/test_gpu_episodes.py holds evaluate_rollout; the sort and press parts add up to the return."""
    import torch

    import marl_sortingenv_amd as M
    from marl_sortingenv_amd.plant import PlantStats

    z = np.load(os.path.join(replay.GOLDEN_DIR, "rule_based_mono_n0_seeds1_10.npz"))
    seeds = z["seeds"]
    assert len(seeds) == 10 and seeds.tolist() == list(range(1, 11))
    env = M.BatchedSortingEnv(kind="mono", num_envs=10, seeds=torch.as_tensor(seeds), max_steps=200, noise_sorting=0.0, balesize=200)
    s, stats = M.evaluate_plant((env, "rule_based"), n_eval_episodes=10, k_steps=50, return_stats=True)
    print(s)
    assert abs(s["mean_reward"] - 44.18) < 0.01 and abs(s["std_reward"] - 1.38) < 0.01
    rows = stats.episodes()
    assert rows.shape == (10, 32) and rows[:, 0].tolist() == [200.0] * 10 and s["length"] == 200.0 and s["episodes"] == 10
    want = z["rewards"].sum(1)
    assert np.max(np.abs(rows[:, 1] - want)) <= 200 * 1e-6  # slot order = env order here; 1e-6: the per-step reward tolerance
    # the same 200 steps traced in one piece: the rows do not depend on how the steps are cut into scans
    env.reset(seeds=env.seeds)
    env.trace_begin_all(200)
    for _ in range(200):
        env.step(env.rule_actions())
    rec = env.trace_end()
    whole = PlantStats(env, 10, slots=1)
    whole.update(rec)
    assert same_bits(whole.episodes(), rows)
    # every step's reward is r_sort + r_press, so over an episode the two partial sums add up to the return within the
    # rounding of three sums of 200 terms: 200 x 2^-52 x sum |r|, the sum over the steps of |reward| + |r_sort| + |r_press|
    rec = rec.cpu().numpy()
    mag = (np.abs(rec[:, R.REWARD]) + np.abs(rec[:, R.R_SORT]) + np.abs(rec[:, R.R_PRESS])).sum(0)
    assert np.all(np.abs(rows[:, 2] + rows[:, 3] - rows[:, 1]) <= 200 * 2.0 ** -52 * mag)
    # the summary's means: the rows' bound, and as much again for the reduction over the ten episodes and the divisions
    assert abs(s["return_sort"] + s["return_press"] - s["return"]) <= 200 * 2.0 ** -52 * mag.sum() / 10
    # the plant quantities are those of the episodes: recomputed from the ledger rows
    assert s["presses_started"] == rows[:, 4:6].sum() / 10 and s["overflow_rate"] == 0.0
    assert s["bales"]["A"] == rows[:, 10].sum() / 10 and s["bales"]["A"] > 0
    assert abs(s["avg_bale_deviation"] - rows[:, 25:30].sum() / (200 * rows[:, 10:15].sum())) <= 1e-15
    # the same evaluation again gives the same bits
    again = M.evaluate_plant((env, "rule_based"), n_eval_episodes=10, k_steps=50)
    np.testing.assert_equal(again, s)  # nested dicts, NaN (no bale of a material) equal to NaN
    # and the random source runs too, with episodes that end by overflow counted as such
    r = M.evaluate_plant((env, "random"), n_eval_episodes=10, k_steps=40, check_overflow=True)
    assert r["episodes"] == 10 and 0.0 <= r["overflow_rate"] <= 1.0 and r["press_noop"] + r["presses_started"] + r["press_busy"] > 0
    env.close()


def test_evaluate_plant_matches_evaluate_policy():
    """The two-launch collector under evaluate_plant and its fused twin under evaluate_policy play the same episodes:
    per episode the plant ledger's float64 return and the float32-row return differ by at most length x 2^-24 x max |reward|,
    the bound include/mse.h states for float32 reward rows."""
    import marl_sortingenv_amd as M

    n_eval = 12
    mk = lambda: M.BatchedSortingEnv(kind="mono", num_envs=5, device=0, base_seed=21, max_steps=7, noise_sorting=0.05,  # noqa: E731
                                     balesize=200)
    pol = M.MlpPolicy.random_init(29, 22, seed=4)
    env_a, env_b = mk(), mk()
    returns, lengths = M.evaluate_policy(M.FusedPolicyRollout(env_a, pol, 4, seed=9), n_eval, deterministic=False,
                                         return_episode_rewards=True)
    col = M.PolicyRolloutCollector(env_b, pol, 4, seed=9)
    col.collect()  # the collector has history: evaluate_plant starts it over
    s, stats = M.evaluate_plant(col, n_eval, return_stats=True)
    rows = stats.episodes(order="time")
    assert rows[:, 0].tolist() == [float(v) for v in lengths]
    bound = np.array(lengths) * 2.0 ** -24 * _max_abs_reward(M, pol)
    print("returns", returns, "plant", rows[:, 1].tolist(), "bound", bound.tolist())
    assert np.all(np.abs(rows[:, 1] - np.array(returns)) <= bound)
    assert abs(s["mean_reward"] - np.mean(returns)) <= bound.max() and s["episodes"] == n_eval
    env_a.close()
    env_b.close()


def _max_abs_reward(M, pol):
    """max |reward| over the steps of the evaluation above, from the float32 rows of the same fused rollouts"""
    env = M.BatchedSortingEnv(kind="mono", num_envs=5, device=0, base_seed=21, max_steps=7, noise_sorting=0.05, balesize=200)
    col = M.FusedPolicyRollout(env, pol, 4, seed=9)
    env.policy_step = 0
    m = 0.0
    for _ in range(-(-3 * 7 // 4)):
        m = max(m, float(col.collect()["rewards"].abs().max()))
    env.close()
    return m
