"""Configs at the edge of the ring kernels' draw budget, and a count of what a step really draws.

k_rollout_ring and k_rollout_policy_roles<RING = true> size their flow control by Params::ring_worst
(max_draws_per_step, csrc/mse_plan.h): the most sort_material draws one step can make, admitted up to
kRingMaxPerStep = 31.  The named configs below sit at 0, 1, 2, 30, 31 and 32, and several of them ATTAIN the bound:
with (1, 1, 1, x) and no boost only the last material mis-sorts, nothing is taken from the pool before it, and a step
of the season with 35 units of D draws exactly 35 - rint(35 x) outputs.

draws_per_step counts the outputs a step consumed by walking the 128-bit LCG from the main stream's state before the
step to its state after (numpy's PCG64: s' = M s + inc).  It reads oracle snapshots only; nothing here calls the
engine."""
import dataclasses

import numpy as np

from tests.config_tables_reference import MASK128, PCG_MULT, max_draws_per_step

RING_MAX_PER_STEP = 31   # kRingMaxPerStep (csrc/mse_device.h)
RING_DEPTH = 64          # kRingDepth: the walk's limit, and the ring's
PRESS_SORT_MODES = (-1, 0, 1, 2, 7)  # Env_2's sort_mode: rule, boost A/C, boost B/D, and two values that boost nothing


@dataclasses.dataclass(frozen=True)
class Budget:
    """One named config: the SortingEnvConfig fields it changes, the ctor noise, and the ring_worst it must compile to
    (`worst`; `worst_press` where Env_2's no-boost mode raises it)."""
    name: str
    fields: dict
    noise: float
    worst: int
    worst_press: int = -1

    def expected_worst(self, kind):
        return self.worst_press if kind == "press" and self.worst_press >= 0 else self.worst

    def sorting_config(self):
        import marl_sortingenv_amd as M

        return M.SortingEnvConfig(**self.fields)

    def oracle_config(self, kind, max_steps, balesize=200):
        """The oracle's struct with the same values (tests/replay.py's oracle_config, for the fields set here)."""
        from oracle.oracle import default_config

        s = self.sorting_config()
        c = default_config(kind, max_steps, self.noise, balesize)
        c.input_batch_size = s.input_batch_size
        c.boost = s.boost
        for m in range(4):
            c.baseline_accuracy[m] = s.baseline_accuracy[m]
        return c

    def struct(self, kind, max_steps=10, **kw):
        return self.sorting_config().to_struct(kind, max_steps=max_steps, noise_sorting=self.noise, balesize=200, **kw)

    def env(self, kind, n, **kw):
        import marl_sortingenv_amd as M

        kw.setdefault("max_steps", 10)
        return M.BatchedSortingEnv(kind=kind, num_envs=n, device=0, noise_sorting=self.noise, balesize=200,
                                   auto_reset=True, config=self.sorting_config(), **kw)

    def oracle(self, kind, n, base_seed=0, max_steps=10):
        from oracle.oracle import OracleBatch

        return OracleBatch(kind, n, base_seed=base_seed, cfg=self.oracle_config(kind, max_steps))


def _only_d(x):
    return dict(baseline_accuracy=(1.0, 1.0, 1.0, x), boost=0.0)


# Default patterns at batch 100: counts (40, 15, 35, 10) and (15, 40, 10, 35).  At batch 120: (48, 18, 42, 12) and
# (18, 48, 12, 42), where 42 - rint(42 x 0.26) = 42 - 11 = 31.
BUDGETS = {b.name: b for b in (
    Budget("W0", dict(baseline_accuracy=(0.99,) * 4, boost=0.0), 0.0, 0),
    Budget("W1", _only_d(0.97), 0.0, 1),
    Budget("W2", dict(baseline_accuracy=(0.97,) * 4, boost=0.0), 0.0, 2),
    Budget("W30", _only_d(0.15), 0.0, 30),
    Budget("W31", _only_d(0.12), 0.0, 31),
    # Env_2's no-boost mode leaves all four stations at 0.62: 15 + 6 + 13 + 4 = 38
    Budget("W31_mixed", dict(baseline_accuracy=(0.62,) * 4, boost=0.25), 0.0, 31, worst_press=38),
    # every station mis-sorts (12 + 5 + 11 + 3): the picks are mixed, so some draws are taken before their station's turn
    Budget("W31_press_noboost", dict(baseline_accuracy=(0.69,) * 4, boost=0.0), 0.0, 31),
    Budget("W32", _only_d(0.09), 0.0, 32),
    # noise 0.05: A..C unboosted fall to 0.95 (2 + 0 draws beside D's) and D to 0.17: 2 + 35 - rint(5.95) = 31
    Budget("W31_noise", dict(baseline_accuracy=(1.0, 1.0, 1.0, 0.22), boost=0.5), 0.05, 31, worst_press=32),
    Budget("W31_batch120", dict(input_batch_size=120, **_only_d(0.26)), 0.0, 31),
)}
RING_ELIGIBLE = tuple(n for n, b in BUDGETS.items() if b.worst <= RING_MAX_PER_STEP)
ATTAINED = ("W1", "W30", "W31", "W31_batch120")  # a step in the season with more D draws exactly ring_worst


def pattern_counts(cfg):
    """[[0] * 4, pattern 1, pattern 2]: floor(ratio * batch) per material (utils/input_generator.py)"""
    return [[0, 0, 0, 0]] + [[int(np.floor(cfg.pattern_ratios[k][m] * cfg.input_batch_size)) for m in range(4)]
                             for k in range(2)]


def reference_worst(cfg, noise, kind):
    """config_tables_reference.max_draws_per_step of a SortingEnvConfig"""
    from marl_sortingenv_amd.config import KIND_BY_NAME

    return max_draws_per_step(list(cfg.baseline_accuracy), cfg.boost, noise, pattern_counts(cfg), KIND_BY_NAME[kind])


def press_sort_modes(n):
    """arange(n) % 5 mapped to PRESS_SORT_MODES, as an int32 numpy array"""
    return np.asarray(PRESS_SORT_MODES, dtype=np.int32)[np.arange(n) % 5]


def _u128(words, at):
    """hi, lo u64 columns -> Python integers (object array)"""
    w = np.asarray(words, dtype=np.uint64)
    return w[..., at].astype(object) * (1 << 64) + w[..., at + 1].astype(object)


def draws_per_step(oracle_env_or_batch, pre_snapshot, post_snapshot):
    """How many outputs of the main stream (snapshot RNG words 0..3: state hi, lo, inc hi, lo) the step between the two
    snapshots consumed: the number of LCG steps s' = M s + inc from the earlier state to the later one.  Snapshots of an
    OracleEnv give an int, of an OracleBatch an int array [N].  Raises if a state is not reached within 64 steps or
    the increment changed (a reseed, not a step)."""
    pre, post = np.asarray(pre_snapshot[2], dtype=np.uint64), np.asarray(post_snapshot[2], dtype=np.uint64)
    n = getattr(oracle_env_or_batch, "num_envs", None)
    assert pre.shape == post.shape == ((30,) if n is None else (n, 30)), (pre.shape, post.shape)
    pre, post = np.atleast_2d(pre), np.atleast_2d(post)
    if not np.array_equal(pre[:, 2:4], post[:, 2:4]):
        raise AssertionError("the main stream's increment changed between the snapshots")
    s, inc, target = _u128(pre, 0), _u128(pre, 2), _u128(post, 0)
    count = np.full(len(s), -1, dtype=np.int64)
    for d in range(RING_DEPTH + 1):
        count[(count < 0) & (s == target)] = d
        if (count >= 0).all():
            break
        s = (s * PCG_MULT + inc) & MASK128
    if (count < 0).any():
        raise AssertionError(f"env {int(np.flatnonzero(count < 0)[0])}: the main stream's state after the step is not "
                             f"within {RING_DEPTH} outputs of its state before")
    return count if n is not None else int(count[0])
