"""Episode accounting and policy evaluation on the device: the reference's unit of measure, cumulative reward per episode.

`EpisodeStats` is SB3's `Monitor` for N envs at once (`mse_episode_scan`): it carries a running return and length per env
across any number of rollouts, closes an episode at every auto-reset inside a rollout, and keeps totals (ep_rew_mean /
ep_len_mean), optionally a ledger of the first episodes per env.  `evaluate_policy` is SB3's function of that name
(src/training.py:149-157,196-209) for a `FusedPolicyRollout`: the first (n_eval_episodes + i) // N episodes of env i
count, the result is np.mean / np.std over them (`mse_episode_summary`).  `evaluate_rollout` does the same for the
built-in action sources of `BatchedSortingEnv.rollout`, the reference's benchmark scenarios.  PyTorch is plumbing
(device memory, zero-fills, the stream, one small copy per result); no torch op computes a sum, and there is no CPU
fallback.  A return is the float64 sum of the float32 rewards the buffers hold (include/mse.h).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import numpy as np
import torch

from ._lib import check, load_library

TOTAL_NAMES = ("episodes", "return_sum", "length_sum", "min_return", "max_return")
SUMMARY_NAMES = ("episodes", "mean_return", "std_return", "mean_length", "min_return", "max_return")


def _ptr(x):
    return None if x is None else C.c_void_p(x.data_ptr())


def eval_targets(n_eval_episodes: int, num_envs: int) -> list:
    """evaluate_policy's episode_count_targets: (n_eval_episodes + i) // num_envs for env i."""
    return [(int(n_eval_episodes) + i) // int(num_envs) for i in range(int(num_envs))]


class EpisodeStats:
    """The carry (running return f64[N] and length i32[N]), the counts i32[N], the totals f64[5], the workspace and, with
    `slots` = E > 0, a ledger of the first E counted episodes per env (f64 / i32 [E, N]).  `targets` (one int per env):
    only the first targets[i] episodes of env i are counted, evaluate_policy's rule; None counts every episode."""

    def __init__(self, num_envs: int, device: int | str | torch.device = 0, slots: int = 0, targets=None):
        if not torch.cuda.is_available():
            raise RuntimeError("EpisodeStats needs a HIP device: there is no CPU fallback")
        self.L = load_library()
        self.num_envs, self.slots = int(num_envs), int(slots)
        if self.num_envs < 1 or self.slots < 0:
            raise ValueError("num_envs must be positive and slots non-negative")
        dev = self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        n, E = self.num_envs, self.slots
        self.run_return = torch.zeros(n, dtype=torch.float64, device=dev)
        self.run_length = torch.zeros(n, dtype=torch.int32, device=dev)
        self.ep_count = torch.zeros(n, dtype=torch.int32, device=dev)
        self.ledger_return = torch.zeros((E, n), dtype=torch.float64, device=dev) if E else None
        self.ledger_length = torch.zeros((E, n), dtype=torch.int32, device=dev) if E else None
        self._totals = torch.zeros(5, dtype=torch.float64, device=dev)
        self._summary = torch.zeros(6, dtype=torch.float64, device=dev)
        self.workspace = torch.empty(int(self.L.mse_episode_workspace_bytes()), dtype=torch.uint8, device=dev)
        self.targets = None
        if targets is not None:
            self.targets = torch.as_tensor(targets).to(device=dev, dtype=torch.int32).contiguous()
            if tuple(self.targets.shape) != (n,):
                raise ValueError("targets must have one entry per env")

    def reset(self) -> None:
        """Forgets everything: carry, counts, ledger and totals are zero-filled."""
        for t in (self.run_return, self.run_length, self.ep_count, self.ledger_return, self.ledger_length, self._totals):
            if t is not None:
                t.zero_()

    def reset_totals(self) -> None:
        """Starts a new window of the totals; the carry, the counts and the ledger stay."""
        self._totals.zero_()

    # ---- checkpoint (checkpoint.py) ----------------------------------------------------------------------------------
    def _state_tensors(self) -> dict:
        return {"run_return": self.run_return, "run_length": self.run_length, "ep_count": self.ep_count,
                "ledger_return": self.ledger_return, "ledger_length": self.ledger_length, "totals": self._totals,
                "targets": self.targets}

    def state_dict(self) -> dict:
        """CPU copies of the carry, the counts, the ledgers, the totals and the targets (None where there is none), with
        `num_envs` / `slots` as the fingerprint."""
        from .checkpoint import cpu

        return dict({k: cpu(t) for k, t in self._state_tensors().items()}, num_envs=self.num_envs, slots=self.slots)

    def check_state_dict(self, sd: dict) -> None:
        """ValueError, with nothing touched, unless `sd` fits: `num_envs` and `slots` equal, every tensor of this
        object's dtype and shape, a ledger exactly where this object has one."""
        from .checkpoint import check_fingerprint, check_tensor

        check_fingerprint({k: sd.get(k) for k in ("num_envs", "slots")}, {"num_envs": self.num_envs, "slots": self.slots},
                          "EpisodeStats")
        for key, t in self._state_tensors().items():
            if key == "targets":
                if sd.get(key) is not None:
                    check_tensor(sd, key, torch.empty(self.num_envs, dtype=torch.int32), "EpisodeStats")
            elif t is None:
                if sd.get(key) is not None:
                    raise ValueError(f"EpisodeStats: the checkpoint has a {key}, this object has no ledger")
            else:
                check_tensor(sd, key, t, "EpisodeStats")

    def load_state_dict(self, sd: dict) -> None:
        self.check_state_dict(sd)
        for key, t in self._state_tensors().items():
            if key != "targets" and t is not None:
                t.copy_(sd[key])
        tg = sd.get("targets")
        self.targets = None if tg is None else tg.to(device=self.device, dtype=torch.int32).contiguous()

    def update(self, data: dict, n_steps: Optional[int] = None) -> None:
        """Accounts one rollout: a collector's dict (`rewards`, `episode_starts`, `last_dones`) or the buffers of
        `BatchedSortingEnv.rollout` (`reward`, `done`).  n_steps: the rows that were filled, if fewer than the buffers
        hold.  Enqueues on the current stream and returns nothing."""
        if "rewards" in data and "episode_starts" in data and "last_dones" in data:
            rewards, dones, starts, last = data["rewards"], None, data["episode_starts"], data["last_dones"]
        elif data.get("reward") is not None and data.get("done") is not None:
            rewards, dones, starts, last = data["reward"], data["done"], None, None
        else:
            raise KeyError("expected rewards / episode_starts / last_dones, or reward / done")
        K = int(rewards.shape[0]) if n_steps is None else int(n_steps)
        if rewards.dim() != 2 or rewards.shape[1] != self.num_envs or not 1 <= K <= rewards.shape[0]:
            raise ValueError(f"rewards must be [K, {self.num_envs}] with 1 <= n_steps <= K")
        for t, dt, shape in ((rewards, torch.float32, rewards.shape), (dones, torch.uint8, rewards.shape),
                             (starts, torch.uint8, rewards.shape), (last, torch.uint8, (self.num_envs,))):
            if t is not None and (t.dtype != dt or tuple(t.shape) != tuple(shape) or not t.is_contiguous() or t.device != self.device):
                raise ValueError("rollout buffers must be contiguous device tensors: f32 rewards, u8 end marks, [K, N] / [N]")
        with torch.cuda.device(self.device):
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            check(self.L.mse_episode_scan(K, self.num_envs, _ptr(rewards), _ptr(dones), _ptr(starts), _ptr(last),
                                          _ptr(self.run_return), _ptr(self.run_length), _ptr(self.ep_count), _ptr(self.targets),
                                          self.slots, _ptr(self.ledger_return), _ptr(self.ledger_length), _ptr(self._totals),
                                          _ptr(self.workspace), stream))

    def totals(self) -> dict:
        """The window's totals (one small device-to-host copy): episodes, return_sum, length_sum, min_return, max_return,
        and mean_return / mean_length, NaN while no episode has ended."""
        v = self._totals.cpu().tolist()
        out = dict(zip(TOTAL_NAMES, v))
        out["episodes"], out["length_sum"] = int(v[0]), int(v[2])
        if v[0] > 0:
            out["mean_return"], out["mean_length"] = v[1] / v[0], v[2] / v[0]
        else:
            out["mean_return"] = out["mean_length"] = out["min_return"] = out["max_return"] = math.nan
        return out

    def summary(self) -> dict:
        """np.mean / np.std (ddof 0) over the ledger's episodes (`mse_episode_summary`, one launch and one small copy)."""
        with torch.cuda.device(self.device):
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            check(self.L.mse_episode_summary(self.num_envs, self.slots, _ptr(self.ep_count), _ptr(self.ledger_return),
                                             _ptr(self.ledger_length), _ptr(self._summary), stream))
        v = self._summary.cpu().tolist()
        out = dict(zip(SUMMARY_NAMES, v))
        out["episodes"] = int(v[0])
        return out

    def episodes(self, order: str = "slot"):
        """(returns f64, lengths i32) numpy arrays of the ledger's episodes.  order="slot": slot-major, envs ascending
        within a slot.  order="time": by the step at which each episode ended, then env - the order in which
        evaluate_policy appends them; it takes the episodes of an env to be back to back from step 0 (a ledger that
        was started together with the envs and holds every episode of an env up to its last one)."""
        if not self.slots:
            raise ValueError("episodes() needs a ledger (slots > 0)")
        cnt = self.ep_count.cpu().numpy()
        ret, length = self.ledger_return.cpu().numpy(), self.ledger_length.cpu().numpy()
        have = np.arange(self.slots)[:, None] < np.minimum(cnt, self.slots)[None, :]
        if order == "slot":
            return ret[have], length[have]
        if order != "time":
            raise ValueError("order must be 'slot' or 'time'")
        ends = np.cumsum(np.where(have, length, 0), axis=0, dtype=np.int64)
        slot, env = np.nonzero(have)
        at = np.lexsort((env, ends[slot, env]))
        return ret[slot[at], env[at]], length[slot[at], env[at]]


def _finish(stats: EpisodeStats, n_eval_episodes: int, return_episode_rewards: bool):
    s = stats.summary()
    if s["episodes"] != int(n_eval_episodes):
        raise RuntimeError(f"{s['episodes']} episodes were counted, not {int(n_eval_episodes)}: an episode ran past max_steps")
    if return_episode_rewards:
        ret, length = stats.episodes(order="time")
        return ret.tolist(), length.tolist()
    return s["mean_return"], s["std_return"]


def _begin(env, n_eval_episodes: int, seeds):
    if int(n_eval_episodes) < 1:
        raise ValueError("n_eval_episodes must be positive")
    if not env.auto_reset:
        raise ValueError("evaluation needs auto_reset=True (episodes end inside a rollout)")
    env.reset(seeds=env.seeds if seeds is None else torch.as_tensor(seeds))
    env.policy_step = 0
    targets = eval_targets(n_eval_episodes, env.num_envs)
    return EpisodeStats(env.num_envs, env.device, slots=max(targets), targets=targets), max(targets)


def evaluate_policy(collector, n_eval_episodes: int = 10, deterministic: bool = True, use_action_masking: bool = True,
                    check_overflow: bool = False, seeds=None, return_episode_rewards: bool = False):
    """SB3's evaluate_policy for a `FusedPolicyRollout`.  The env is reset (`seeds`, else the env's own `seeds`) and
    its policy step counter set to 0, so the result is a function of weights, config and seeds.  Env i contributes its
    first (n_eval_episodes + i) // N episodes.  ceil(max target * max_steps / K) collect + scan pairs are enqueued with
    no host synchronisation between them (no episode of the reference outlasts max_steps), then one summary and one copy.
    Returns (mean, std) of the episode returns, or (returns, lengths) in SB3's order with return_episode_rewards."""
    env = collector.env
    stats, most = _begin(env, n_eval_episodes, seeds)
    K = collector.n_steps
    for _ in range(-(-most * env.max_steps // K)):
        stats.update(collector.collect(deterministic=deterministic, use_action_masking=use_action_masking,
                                       check_overflow=check_overflow))
    return _finish(stats, n_eval_episodes, return_episode_rewards)


def evaluate_rollout(env, policy: str = "rule_based", n_eval_episodes: int = 10, k_steps: int = 50, policy_seed: int = 2024,
                     use_action_masking: bool = True, check_overflow: bool = False, seeds=None,
                     return_episode_rewards: bool = False, sort_agent=None, press_agent=None, press_agent_maskable: bool = True):
    """`evaluate_policy` for the action sources of `BatchedSortingEnv.rollout`: policy = "rule_based" | "random" |
    "model" (with its optional agents) - the reference's benchmark scenarios, k_steps per launch."""
    if policy not in ("rule_based", "random", "model"):
        raise ValueError("policy must be 'rule_based', 'random' or 'model'")
    stats, most = _begin(env, n_eval_episodes, seeds)
    K = int(k_steps)
    buf = env.alloc_rollout(K, obs=False, mask=False)
    extra = dict(sort_agent=sort_agent, press_agent=press_agent, press_agent_maskable=press_agent_maskable) if policy == "model" else {}
    for _ in range(-(-most * env.max_steps // K)):
        env.rollout(K, policy_seed=policy_seed, buffers=buf, use_action_masking=use_action_masking, check_overflow=check_overflow,
                    policy=policy, **extra)
        stats.update(buf)
    return _finish(stats, n_eval_episodes, return_episode_rewards)
