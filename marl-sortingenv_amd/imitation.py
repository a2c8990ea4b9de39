"""Behaviour cloning of the env's rule-based controller on the device: a supervised start for PPO.

`DemonstrationCollector` steps N envs and records, per step, the row a learner's policy would be shown and the action
the reference's rule-based controller (`sorting_rules()` / `check_container_level()`, `mse_rule_actions`) takes in that
state.  `ImitationLearner` minimises the cross-entropy of those labels under the policy's masked softmax (plus SB3's
entropy bonus and, with `returns`, the critic's squared error on the discounted reward-to-go): per minibatch one
`mse_bc_loss_grad` (two launches: the behaviour-cloning instantiation of the learner's gradient kernel, then its
reduction) and one `mse_ppo_adam_step`, with `PPOLearner`'s shuffle keys, Adam kernel and weight hand-over.  A
`PPOLearner` constructed afterwards on the same policy continues from the cloned weights.  PyTorch is plumbing (device
memory, the stream, the copies into the buffers, and for the modular agents the integer split of the rule's flat action
into a // 11 and a % 11); there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import torch

from ._lib import (DEMO_BUFFER_NAMES, MSE_DEMO_ACTOR_DETERMINISTIC, MSE_PREVIEW_DETERMINISTIC, MSE_STEP_CHECK_OVERFLOW,
                   PREVIEW_BUFFER_NAMES, MseDemoBuffers, MsePreviewBuffers, check)
from .batched import BatchedSortingEnv
from .collector import rollout_buffers
from .learner import PPOLearner, _ptr, _stream, training_loop
from .policy import MlpPolicy

BC_STAT_NAMES = ("loss", "bc_loss", "value_loss", "entropy_loss", "accuracy", "unusable", "_", "_")
AGENT_DIMS = {"sort": (13, 2), "press": (16, 11), "preview": (29, 22)}
DEMO_ROWS = ("observations", "action_masks", "actions", "stepped_actions", "rewards", "episode_starts", "returns")
FUSED_DEMO_ROWS = ("observations", "action_masks", "actions", "stepped_actions", "expert_stepped", "rewards", "episode_starts",
                   "last_dones", "returns")


class DemonstrationCollector:
    """K steps of N envs with the rule-based controller as the teacher.  Per step, in the order the reference's
    `mode='rule_based'` acts:

    1. the observation: `env.obs` / `env.mask` for agent="own" (a policy of the env's own dimensions); on a "mono" env
       `sort_agent_obs()` and no mask for agent="sort" (13 -> 2), `press_agent_obs()` and `mask[:, :11]` for
       agent="press" (16 -> 11), `mono_agent_obs()` - the mono policy's in-step view, both previews in one row - and
       the full `env.mask` for agent="preview" (29 -> 22);
    2. the label: `env.rule_actions()` - the flat action a for "own" and "preview", a // 11 for "sort", a % 11 for "press";
    3. the step: with actor=None the expert's action is stepped.  With an `MlpPolicy` as `actor` that policy's action
       (sampled with `seed`, or its argmax with deterministic_actor=True) is stepped and the expert's action stays the
       label - on-policy relabelling; for "sort" / "press" the other half of the flat action stays the expert's.

    `collect()` returns contiguous [K, N, ...] device tensors under `PPOLearner`'s names: `observations`,
    `action_masks` (None for "sort"), `actions` (the labels), `rewards`, `episode_starts`, `last_dones`, `returns`, and
    `stepped_actions` (the flat actions the envs were stepped with).  `returns` is `mse_gae` with zero values and
    lambda = 1: the discounted reward-to-go INSIDE the window, cut at episode ends, with NO bootstrap at the window's
    end - the last rows of a window see only the rewards left in it."""

    def __init__(self, env: BatchedSortingEnv, n_steps: int, agent: str = "own", actor: Optional[MlpPolicy] = None,
                 deterministic_actor: bool = False, gamma: float = 0.99, seed: int = 2024):
        if agent not in ("own", "sort", "press", "preview"):
            raise ValueError(f"agent must be 'own', 'sort', 'press' or 'preview', not {agent!r}")
        if agent != "own" and env.kind != "mono":
            raise ValueError(f"agent={agent!r} is an in-step view of Env_3: it needs a 'mono' env")
        if not env.auto_reset:
            raise ValueError("collection needs auto_reset=True (episodes end inside a rollout)")
        self.obs_dim, self.n_actions = (env.obs_dim, env.num_actions) if agent == "own" else AGENT_DIMS[agent]
        if actor is not None and (actor.obs_dim != self.obs_dim or actor.n_actions != self.n_actions):
            raise ValueError(f"the actor must be a {self.obs_dim} -> {self.n_actions} policy")
        self.env, self.agent, self.actor = env, agent, actor
        self.deterministic_actor, self.gamma = bool(deterministic_actor), float(gamma)
        self.n_steps, self.seed, self.t = int(n_steps), int(seed), 0
        n, K, dev = env.num_envs, self.n_steps, env.device
        self.buffers = rollout_buffers(env, K, names=DEMO_ROWS, dims=(self.obs_dim, self.n_actions))
        if agent == "sort":
            self.buffers["action_masks"] = None  # the sorter is not maskable
        self._zeros = torch.zeros((K + 1, n), dtype=torch.float32, device=dev)  # mse_gae's values and last_values
        self._adv = torch.empty((K, n), dtype=torch.float32, device=dev)
        self._last_done = torch.ones((n,), dtype=torch.uint8, device=dev)  # the envs were just reset
        self._out = None

    def _view(self):
        env = self.env
        if self.agent == "own":
            return env.obs, env.mask
        if self.agent == "sort":
            return env.sort_agent_obs(), None
        if self.agent == "preview":
            return env.mono_agent_obs(), env.mask
        return env.press_agent_obs(), env.mask[:, :11]  # press_action_masks()

    def collect(self) -> dict:
        env, b, K = self.env, self.buffers, self.n_steps
        for k in range(K):
            obs, mask = self._view()
            b["observations"][k].copy_(obs)
            if mask is not None:
                b["action_masks"][k].copy_(mask)
            b["episode_starts"][k].copy_(self._last_done)
            rule = env.rule_actions()
            label = rule if self.agent in ("own", "preview") else (rule // 11 if self.agent == "sort" else rule % 11)
            b["actions"][k].copy_(label)
            if self.actor is None:
                stepped = rule
            else:
                self._out = self.actor.forward(obs, mask, seed=self.seed, t=self.t, deterministic=self.deterministic_actor,
                                               index_offset=env.index_offset, out=self._out)
                a = self._out["action"]
                stepped = a if self.agent in ("own", "preview") else (11 * a + rule % 11 if self.agent == "sort" else rule - rule % 11 + a)
            b["stepped_actions"][k].copy_(stepped)
            _, rew, done, _ = env.step(b["stepped_actions"][k])
            b["rewards"][k].copy_(rew)
            self._last_done.copy_(done)
            self.t += 1
        last_dones = self._last_done.clone()
        with torch.cuda.device(env.device):
            check(env.L.mse_gae(K, env.num_envs, _ptr(b["rewards"]), _ptr(self._zeros), _ptr(b["episode_starts"]),
                                _ptr(self._zeros[K]), _ptr(last_dones), self.gamma, 1.0, _ptr(self._adv), _ptr(b["returns"]),
                                _stream(env.device)))
        return dict(b, last_dones=last_dones)


def expert_threshold(beta: float) -> int:
    """The integer `mse_rollout_demo` compares a draw's upper 24 bits with: int(round(beta * 2**24)), in [0, 2**24].
    beta is the share of (env, step) pairs in which the expert's action is stepped; NaN and values outside [0, 1] are
    refused."""
    b = float(beta)
    if math.isnan(b) or not 0.0 <= b <= 1.0:
        raise ValueError(f"beta must be in [0, 1], not {beta!r}")
    return int(round(b * 2 ** 24))


class FusedDemonstrationRollout:
    """`DemonstrationCollector(agent="own")` in one launch (`mse_rollout_demo`): per step the expert labels the state,
    the student `actor` acts on it (sampled with `seed`, or its argmax with deterministic_actor=True), and per env and
    step the expert's action is stepped with probability `beta`, else the student's - the beta-mixture of DAgger, decided
    by a word of `mix_seed`'s stream against `expert_threshold(beta)`.  beta = 0 is `DemonstrationCollector(actor=
    student)`, beta = 1 steps what `DemonstrationCollector(actor=None)` steps.  `beta` may be set between calls; with
    actor=None it must be 1.

    `collect()` is that launch plus the one `mse_gae` launch for `returns`, and returns `DemonstrationCollector`'s dict
    (`observations`, `action_masks`, `actions` = the labels, `stepped_actions`, `rewards`, `episode_starts`,
    `last_dones`, `returns`) plus `expert_stepped` u8[K, N]; the buffers are allocated once.  The modular views ("sort" /
    "press" on Env_3) have a launch of their own: `FusedModularRollout(expert_labels=True).demo_view(who)`.  The env's own obs / mask tensors are not refreshed.

    agent="preview" (a "mono" env, a 29 -> 22 actor): `DemonstrationCollector(agent="preview")` in one launch
    (`mse_rollout_policy_preview`) - the student is shown `mono_agent_obs()`, the observation after the step's flow update.
    That kernel always carries a network: actor=None is refused."""

    def __init__(self, env: BatchedSortingEnv, n_steps: int, actor: Optional[MlpPolicy] = None,
                 deterministic_actor: bool = False, beta: Optional[float] = None, gamma: float = 0.99, seed: int = 2024,
                 mix_seed: Optional[int] = None, check_overflow: bool = False, agent: str = "own"):
        if agent not in ("own", "preview"):
            raise ValueError(f"agent must be 'own' or 'preview', not {agent!r}")
        if agent == "preview" and env.kind != "mono":
            raise ValueError("agent='preview' is the mono policy's in-step view of Env_3: it needs a 'mono' env")
        if agent == "preview" and actor is None:
            raise ValueError("agent='preview' with actor=None: mse_rollout_policy_preview always carries a network; collect the "
                             "expert's own demonstrations with DemonstrationCollector(agent='preview')")
        if not env.auto_reset:
            raise ValueError("collection needs auto_reset=True (episodes end inside a rollout)")
        if int(n_steps) < 1:
            raise ValueError("n_steps must be >= 1")
        if actor is not None and (actor.obs_dim != env.obs_dim or actor.n_actions != env.num_actions):
            raise ValueError(f"the actor must be a {env.obs_dim} -> {env.num_actions} policy")
        self.env, self.actor, self.agent = env, actor, agent
        self.deterministic_actor, self.gamma, self.check_overflow = bool(deterministic_actor), float(gamma), bool(check_overflow)
        self.n_steps, self.seed = int(n_steps), int(seed)
        self.mix_seed = self.seed + 1 if mix_seed is None else int(mix_seed)
        if actor is not None and self.mix_seed == self.seed:
            raise ValueError("mix_seed == seed: who steps and what the actor draws would come from one word")
        self.beta = (1.0 if actor is None else 0.0) if beta is None else beta
        n, K, dev = env.num_envs, self.n_steps, env.device
        self.buffers = rollout_buffers(env, K, names=FUSED_DEMO_ROWS)
        self._zeros = torch.zeros((K + 1, n), dtype=torch.float32, device=dev)  # mse_gae's values and last_values
        self._adv = torch.empty((K, n), dtype=torch.float32, device=dev)
        b = self.buffers
        if agent == "preview":  # the labels go to `actions`; the student's own draws, log-probabilities and values are not kept
            rows = {"expert_actions": b["actions"], **{k: b[k] for k in PREVIEW_BUFFER_NAMES if k in b and k != "actions"}}
            self._out = MsePreviewBuffers(C.sizeof(MsePreviewBuffers), 0,
                                          *(rows[name].data_ptr() if name in rows else None for name in PREVIEW_BUFFER_NAMES))
        else:
            self._out = MseDemoBuffers(C.sizeof(MseDemoBuffers), 0, *(b["actions" if name == "labels" else name].data_ptr()
                                                                       for name in DEMO_BUFFER_NAMES))

    @property
    def beta(self) -> float:
        return self._beta

    @beta.setter
    def beta(self, value: float) -> None:
        threshold = expert_threshold(value)
        if self.actor is None and threshold != 2 ** 24:
            raise ValueError("without an actor the expert always steps: beta must be 1")
        self._beta, self._threshold = float(value), threshold

    def collect(self) -> dict:
        env, b, K = self.env, self.buffers, self.n_steps
        preview = self.agent == "preview"
        flags = (MSE_STEP_CHECK_OVERFLOW if self.check_overflow else 0) | \
                ((MSE_PREVIEW_DETERMINISTIC if preview else MSE_DEMO_ACTOR_DETERMINISTIC) if self.deterministic_actor else 0)
        with torch.cuda.device(env.device):
            if preview:
                check(env.L.mse_rollout_policy_preview(env._h, self.actor._h, K, self.seed, self.mix_seed, self._threshold,
                                                       flags, C.byref(self._out), env._stream()))
            else:
                check(env.L.mse_rollout_demo(env._h, None if self.actor is None else self.actor._h, K, self.seed, self.mix_seed,
                                             self._threshold, flags, C.byref(self._out), env._stream()))
            check(env.L.mse_gae(K, env.num_envs, _ptr(b["rewards"]), _ptr(self._zeros), _ptr(b["episode_starts"]),
                                _ptr(self._zeros[K]), _ptr(b["last_dones"]), self.gamma, 1.0, _ptr(self._adv), _ptr(b["returns"]),
                                env._stream()))
        return b


class ImitationLearner(PPOLearner):
    """Supervised learning of demonstrated actions with the learner's own kernels.  The loss of a minibatch is

        bc_loss + ent_coef * entropy_loss + vf_coef * value_loss

    with bc_loss the mean of -log pi(label | row) under the masked softmax (a row whose label the mask forbids counts 0
    and is reported in `unusable`), entropy_loss SB3's, and value_loss the mean squared error of the critic against
    `data["returns"]` (absent or None: the critic is left alone, its gradient is exactly 0).  The optimiser state, the
    shuffle (`shuffle`, keyed by `seed` and the epochs of the learner's lifetime), `weight_sync` and `arithmetic` are
    `PPOLearner`'s, whose `adam_step`, `permutation` and hand-over this class inherits.  Checkpointing is not offered:
    `state_dict` / `load_state_dict` raise."""

    def __init__(self, policy: MlpPolicy, learning_rate: float = 1e-3, n_epochs: int = 1, batch_size: Optional[int] = None,
                 ent_coef: float = 0.0, vf_coef: float = 0.5, max_grad_norm: float = 0.5, adam_eps: float = 1e-5,
                 seed: int = 0, shuffle: str = "cpu", weight_sync: str = "host", arithmetic: str = "fma", exchange=None):
        if exchange is not None:
            raise ValueError("ImitationLearner cannot be combined with an exchange: mse_bc_loss_grad has no sharded form")
        super().__init__(policy, learning_rate=float(learning_rate), n_epochs=n_epochs, batch_size=batch_size, ent_coef=ent_coef,
                         vf_coef=vf_coef, max_grad_norm=max_grad_norm, normalize_advantage=False, adam_eps=adam_eps, seed=seed,
                         shuffle=shuffle, weight_sync=weight_sync, arithmetic=arithmetic)

    def loss_grad(self, data: dict, rows: Optional[torch.Tensor], batch: int, stats_out: torch.Tensor,
                  weights: Optional[torch.Tensor] = None, grad_out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One `mse_bc_loss_grad` on the flattened rows of `data` (`observations`, `actions` = the labels, optional
        `action_masks` and `returns`); returns the gradient tensor.  rows: i64 device tensor of row indices, or None
        for rows 0 .. batch - 1.  stats_out: f32[8] on the device, columns BC_STAT_NAMES."""
        p = self.policy
        obs = data["observations"]
        n_rows = obs.shape[0] * obs.shape[1] if obs.dim() == 3 else obs.shape[0]
        mask, ret = data.get("action_masks"), data.get("returns")
        w = self.weights if weights is None else weights
        g = self.grad if grad_out is None else grad_out
        for name, t, dtype in (("observations", obs, torch.float32), ("actions", data["actions"], torch.int32),
                               ("action_masks", mask, torch.uint8), ("returns", ret, torch.float32)):
            if t is not None and (not t.is_contiguous() or t.dtype != dtype):
                raise ValueError(f"{name} must be contiguous {dtype}")
        with torch.cuda.device(self.device):
            check(self.L.mse_bc_loss_grad(p.obs_dim, p.n_actions, _ptr(w), n_rows, _ptr(rows), int(batch), _ptr(obs), _ptr(mask),
                                          _ptr(data["actions"]), _ptr(ret), C.byref(self.params), _ptr(g), _ptr(stats_out),
                                          _ptr(self.workspace), _stream(self.device), 1 if self.arithmetic == "matrix" else 0))
        return g

    def update(self, data: dict) -> dict:
        """n_epochs passes over a permutation of the K * N rows of `data` (`PPOLearner.update`'s loop: the same shuffle
        keys, a short last minibatch, one loss_grad + adam_step per minibatch without a host synchronisation), then the
        hand-over of the weights to the policy.  Returns {"stats": f32[n_minibatches, 8] (device; columns
        BC_STAT_NAMES), "mean": {name: float}}."""
        obs = data["observations"]
        total = obs.shape[0] * obs.shape[1] if obs.dim() == 3 else obs.shape[0]
        bs = self.batch_size if self.batch_size is not None else (total + 3) // 4
        bs = max(1, min(int(bs), total))
        n_mb = self.n_epochs * ((total + bs - 1) // bs)
        stats = torch.zeros((n_mb, 8), dtype=torch.float32, device=self.device)
        for i, rows in enumerate(self._minibatches(total, bs)):
            self.loss_grad(data, rows, rows.numel(), stats[i])
            self.adam_step()
        self._hand_over()
        mean = stats.mean(dim=0).cpu().tolist()
        self.policy.sync()
        return {"stats": stats, "mean": dict(zip(BC_STAT_NAMES, mean))}

    def learn(self, collector, iterations: int, callback=None, eval_collector=None, eval_freq: int = 0,
              n_eval_episodes: int = 10, beta=None) -> list:
        """Alternates `collector.collect()` (a `DemonstrationCollector` or `FusedDemonstrationRollout`; one whose `actor`
        is this learner's policy relabels the states the clone itself visits) and `update()`; returns the per-iteration
        mean statistics, each with the collection's mean reward per env-step under "reward".  eval_collector (a
        `FusedPolicyRollout` over this learner's policy and an env of its own) with eval_freq > 0: every eval_freq-th
        record gains `eval_mean_reward` and `eval_std_reward` from `evaluate_policy(eval_collector, n_eval_episodes)`.
        beta (a `FusedDemonstrationRollout`'s mixture): a number, or a function of the fraction of iterations done
        (it / iterations, from 0 towards 1); it is written into `collector.beta` before each `collect()`, and each record
        then carries `beta` and, under "expert_share", the share of rows the expert stepped.  None: nothing is set and
        the records are as before."""
        def collect(it):
            if beta is not None:
                collector.beta = float(beta(it / int(iterations)) if callable(beta) else beta)
            return collector.collect()

        def step(data, progress_remaining):
            rec = dict(self.update(data)["mean"], reward=float(data["rewards"].mean()))
            if beta is not None:
                rec.update(beta=collector.beta, expert_share=float(data["expert_stepped"].float().mean()))
            return rec

        return training_loop(iterations, collect, step, evaluate=self._evaluator(eval_collector, eval_freq, n_eval_episodes),
                             eval_freq=eval_freq, callback=callback)

    def state_dict(self) -> dict:
        raise NotImplementedError("ImitationLearner is not checkpointed: save the policy's state_dict()")

    def load_state_dict(self, sd: dict, strict: bool = True) -> None:
        raise NotImplementedError("ImitationLearner is not checkpointed: load the weights into the policy")
