"""Plant ledger for every env: what the reference's dashboard reads off one env, per episode and for all N at once.

`BatchedSortingEnv.trace_begin_all` makes every `step()` store the trace record of every env (`mse_trace_begin_all`);
`PlantStats` folds such records into one row of `MSE_PLANT_COLS` doubles per episode (`mse_plant_scan`): length, the return
and its sorting / pressing parts, the press log's counts, overflow, what was left in the containers, and per material the
bales, their mass, quality and |size - standard size| by the reference's merge rule (env_super.py:661-687).  It is shaped
like `EpisodeStats`: a carry across calls, counts, optional per-env targets and ledger, totals.  `evaluate_plant` runs an
evaluation through it.  PyTorch is plumbing (device memory, zero-fills, the stream, small copies); the sums are the
kernel's, and there is no CPU fallback.  include/mse.h documents the columns.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import numpy as np
import torch

from ._lib import MSE_PLANT_COLS, MSE_PLANT_RUN_COLS, MSE_TRACE_COLS, check, load_library
from .episodes import eval_targets

MATERIALS = ("A", "B", "C", "D", "E")
COLUMN_NAMES = ("length", "return", "return_sort", "return_press", "press1_started", "press2_started", "press_busy", "press_noop",
                "overflow", "left_over") + tuple(f"{what}_{m}" for what in ("bales", "bale_mass", "bale_quality_sum", "bale_deviation_sum")
                                                 for m in MATERIALS) + ("reserved0", "reserved1")


def _ptr(x):
    return None if x is None else C.c_void_p(x.data_ptr())


def plant_params(env) -> tuple:
    """(bale_standard_size, floor(bale_standard_size * bale_remainder_threshold)) of a `BatchedSortingEnv` (mse_plant_params)."""
    out = (C.c_int32 * 2)()
    check(env.L.mse_plant_params(env._h, C.byref(out)))
    return int(out[0]), int(out[1])


class PlantStats:
    """The carry f64[MSE_PLANT_RUN_COLS, N], the counts i32[N], the totals f64[1 + MSE_PLANT_COLS], the workspace and, with
    `slots` = E > 0, a ledger f64[E, MSE_PLANT_COLS, N] of the first E counted episodes per env.  `env_or_params`: a
    `BatchedSortingEnv` (its compiled config and device are used) or (bale_standard_size, remainder_units).  `targets` (one
    int per env): only the first targets[i] episodes of env i are counted; None counts every episode."""

    def __init__(self, env_or_params, num_envs: int, slots: int = 0, targets=None, device: int | str | torch.device | None = None):
        if not torch.cuda.is_available():
            raise RuntimeError("PlantStats needs a HIP device: there is no CPU fallback")
        self.L = load_library()
        if hasattr(env_or_params, "_h"):
            self.bale_standard_size, self.remainder_units = plant_params(env_or_params)
            device = env_or_params.device if device is None else device
        else:
            self.bale_standard_size, self.remainder_units = (int(v) for v in env_or_params)
        device = 0 if device is None else device
        self.num_envs, self.slots = int(num_envs), int(slots)
        if self.num_envs < 1 or self.slots < 0:
            raise ValueError("num_envs must be positive and slots non-negative")
        dev = self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        n, E = self.num_envs, self.slots
        self.run = torch.zeros((MSE_PLANT_RUN_COLS, n), dtype=torch.float64, device=dev)
        self.ep_count = torch.zeros(n, dtype=torch.int32, device=dev)
        self.ledger = torch.zeros((E, MSE_PLANT_COLS, n), dtype=torch.float64, device=dev) if E else None
        self._totals = torch.zeros(1 + MSE_PLANT_COLS, dtype=torch.float64, device=dev)
        self.workspace = torch.empty(int(self.L.mse_plant_workspace_bytes()), dtype=torch.uint8, device=dev)
        self.targets = None
        if targets is not None:
            self.targets = torch.as_tensor(targets).to(device=dev, dtype=torch.int32).contiguous()
            if tuple(self.targets.shape) != (n,):
                raise ValueError("targets must have one entry per env")

    def reset(self) -> None:
        """Forgets everything: carry, counts, ledger and totals are zero-filled."""
        for t in (self.run, self.ep_count, self.ledger, self._totals):
            if t is not None:
                t.zero_()

    def update(self, records: torch.Tensor) -> None:
        """Accounts the steps of `records` f64[K, MSE_TRACE_COLS, N] (`trace_records()` of an all-env trace).  Enqueues on
        the current stream and returns nothing."""
        if records.dim() != 3 or tuple(records.shape[1:]) != (MSE_TRACE_COLS, self.num_envs) or records.shape[0] < 1:
            raise ValueError(f"records must be [K >= 1, {MSE_TRACE_COLS}, {self.num_envs}]")
        if records.dtype != torch.float64 or not records.is_contiguous() or records.device != self.device:
            raise ValueError("records must be a contiguous float64 device tensor")
        with torch.cuda.device(self.device):
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            check(self.L.mse_plant_scan(int(records.shape[0]), self.num_envs, _ptr(records), self.bale_standard_size,
                                        self.remainder_units, _ptr(self.run), _ptr(self.ep_count), _ptr(self.targets), self.slots,
                                        _ptr(self.ledger), _ptr(self._totals), _ptr(self.workspace), stream))

    def totals(self) -> dict:
        """The totals (one small device-to-host copy): `episodes` and the sum of every column under COLUMN_NAMES
        (`overflow`: the episodes that ended in one)."""
        v = self._totals.cpu().tolist()
        out = {"episodes": int(v[0])}
        out.update(zip(COLUMN_NAMES[:30], v[1:31]))
        return out

    def summary(self) -> dict:
        """Per-episode means over the counted episodes, from the totals: `return`, `return_sort`, `return_press`, `length`,
        `presses_started`, `press_busy`, `press_noop`, `overflow_rate`, `left_over`; `bales`, `bale_mass` per episode and
        `bale_quality` (mean over bales, a fraction) as dicts by material; `avg_bale_deviation`, the reference's
        _calculate_avg_bale_deviation over all counted bales.  NaN where there is nothing to average."""
        t = self.totals()
        n = t["episodes"]

        def per(x, d):
            return x / d if d > 0 else math.nan

        out = {"episodes": n}
        for key, col in (("return", "return"), ("return_sort", "return_sort"), ("return_press", "return_press"), ("length", "length"),
                         ("press_busy", "press_busy"), ("press_noop", "press_noop"), ("overflow_rate", "overflow"),
                         ("left_over", "left_over")):
            out[key] = per(t[col], n)
        out["presses_started"] = per(t["press1_started"] + t["press2_started"], n)
        out["bales"] = {m: per(t[f"bales_{m}"], n) for m in MATERIALS}
        out["bale_mass"] = {m: per(t[f"bale_mass_{m}"], n) for m in MATERIALS}
        out["bale_quality"] = {m: per(t[f"bale_quality_sum_{m}"] / 100.0, t[f"bales_{m}"]) for m in MATERIALS}
        bales = sum(t[f"bales_{m}"] for m in MATERIALS)
        out["avg_bale_deviation"] = per(sum(t[f"bale_deviation_sum_{m}"] for m in MATERIALS), self.bale_standard_size * bales)
        return out

    def episodes(self, order: str = "slot") -> np.ndarray:
        """The ledger's episodes as rows f64[M, MSE_PLANT_COLS].  order="slot": slot-major, envs ascending within a slot.
        order="time": by the step at which each episode ended, then env (it takes the episodes of an env to be back to
        back from step 0, as `EpisodeStats.episodes` does)."""
        if not self.slots:
            raise ValueError("episodes() needs a ledger (slots > 0)")
        cnt = self.ep_count.cpu().numpy()
        led = self.ledger.cpu().numpy()
        have = np.arange(self.slots)[:, None] < np.minimum(cnt, self.slots)[None, :]
        slot, env = np.nonzero(have)
        if order == "time":
            ends = np.cumsum(np.where(have, led[:, 0, :], 0.0), axis=0)
            at = np.lexsort((env, ends[slot, env]))
            slot, env = slot[at], env[at]
        elif order != "slot":
            raise ValueError("order must be 'slot' or 'time'")
        return led[slot, :, env]


def _collector_env(source):
    if isinstance(source, tuple):
        env, name = source
        if name not in ("random", "rule_based"):
            raise ValueError("a built-in source is (env, 'random') or (env, 'rule_based')")
        return env, name
    return source.env, None


def evaluate_plant(source, n_eval_episodes: int = 10, k_steps: Optional[int] = None, seeds=None, policy_seed: int = 2024,
                   use_action_masking: bool = True, check_overflow: bool = False, collect_kwargs: Optional[dict] = None,
                   return_stats: bool = False):
    """`evaluate_policy`'s protocol with the plant ledger as the result.  `source`: a collector that steps through
    `BatchedSortingEnv.step` (`PolicyRolloutCollector`, `ModelRolloutCollector`, `ModularRolloutCollector`,
    `DemonstrationCollector`; `collect_kwargs` go to its `collect`) or `(env, "random" | "rule_based")`, stepped with
    `sample_actions(policy_seed)` / `rule_actions()` and `step(use_action_masking=, check_overflow=)`.  The fused rollouts do
    not record; their multi-launch twins are what this diagnostic runs.  The env is reset (`seeds`, else its own), its
    policy step counter and the collector's are set to 0; env i contributes its first (n_eval_episodes + i) // N episodes.
    Per collection of K steps (the collector's `n_steps`, else `k_steps`, default 50) an all-env trace of K steps is
    attached, scanned and begun again: K x 40 x N doubles of device memory.  Returns `PlantStats.summary()` plus
    `mean_reward` / `std_reward`, np.mean / np.std (ddof 0) over the ledger's returns (column 1) - with return_stats, also
    the PlantStats."""
    env, builtin = _collector_env(source)
    if int(n_eval_episodes) < 1:
        raise ValueError("n_eval_episodes must be positive")
    if not env.auto_reset:
        raise ValueError("evaluation needs auto_reset=True (episodes end inside a collection)")
    kwargs = dict(collect_kwargs or {})
    K = int(getattr(source, "n_steps", 0) or (k_steps if k_steps is not None else 50))
    if K < 1:
        raise ValueError("k_steps must be positive")
    env.reset(seeds=env.seeds if seeds is None else torch.as_tensor(seeds))
    env.policy_step = 0
    if builtin is None:
        if hasattr(source, "t"):
            source.t = 0
        if getattr(source, "_last_done", None) is not None:
            source._last_done.fill_(1)  # the envs were just reset
    targets = eval_targets(n_eval_episodes, env.num_envs)
    most = max(targets)
    stats = PlantStats(env, env.num_envs, slots=most, targets=targets)
    try:
        for _ in range(-(-most * env.max_steps // K)):
            env.trace_begin_all(K)
            if builtin is None:
                source.collect(**kwargs) if hasattr(source, "n_steps") else source.collect(K, **kwargs)
            else:
                for _k in range(K):
                    actions = env.rule_actions() if builtin == "rule_based" else env.sample_actions(policy_seed)
                    env.step(actions, use_action_masking=use_action_masking, check_overflow=check_overflow)
            stats.update(env.trace_records())
    finally:
        env.trace_end()
    out = stats.summary()
    if out["episodes"] != int(n_eval_episodes):
        raise RuntimeError(f"{out['episodes']} episodes were counted, not {int(n_eval_episodes)}: an episode ran past max_steps")
    returns = stats.episodes()[:, 1]
    out["mean_reward"], out["std_reward"] = float(np.mean(returns)), float(np.std(returns))
    return (out, stats) if return_stats else out


def format_summary(s: dict) -> str:
    """A few lines of text for a summary dict (the tools print it beside the reward)."""
    lines = [f"episodes {s['episodes']}  return {s['return']:.3f} = sort {s['return_sort']:.3f} + press {s['return_press']:.3f}"
             f"  length {s['length']:.1f}",
             f"presses started {s['presses_started']:.2f}  busy/invalid {s['press_busy']:.2f}  no-op {s['press_noop']:.2f}"
             f"  overflow rate {s['overflow_rate']:.3f}  left over {s['left_over']:.1f}",
             "bales " + "  ".join(f"{m} {s['bales'][m]:.2f} (mass {s['bale_mass'][m]:.0f}, q {s['bale_quality'][m]:.2f})" for m in MATERIALS),
             f"avg bale deviation {s['avg_bale_deviation']:.4f}"]
    return "\n".join(lines)
