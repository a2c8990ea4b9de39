"""On-device rollout collection with a learned policy (the caller side of the path).

SB3's `collect_rollouts` (the loop inside `model.learn`, src/training.py:191) alternates policy forward and
`env.step` on the host, one env at a time.  `PolicyRolloutCollector` does the same alternation for N envs with both
halves on the device - `mse_policy_forward` then `mse_step` - and fills buffers shaped like SB3's
`MaskableRolloutBuffer` ([K, N, ...]: observations, action masks, actions, log-probabilities, values, rewards,
episode starts), so a learner can consume them without a host copy.  For `Env_2_Pressing` an optional sorting policy
(13 -> 2, evaluated deterministically on `mse_sort_agent_obs`, env_2_press.py:101-104) plays the pre-trained sorting
agent.  Two launches per step.

`FusedPolicyRollout` is the same collection in ONE launch per rollout (`mse_rollout_policy`): the policy forward runs
inside the rollout kernel, the observation never leaves the wave's registers between the env transition and the
policy's MFMA chain.  Its buffers are bit-identical to `PolicyRolloutCollector`'s for the same seed.

`ModelRolloutCollector` is Env_3_Monolith.step(action=None, mode='model') (env_monolith.py:186-221) for N envs in
several launches per step: the agents' previews, their forwards, the env's own fallback draws, the step.  It is what
`BatchedSortingEnv.rollout(K, policy="model")` (`mse_rollout_model`, one launch per rollout) is held against, and it
serves the handles that kernel refuses (literal_choice, general generator mode).

`FusedModularRollout` collects for BOTH modular agents at once in Env_3 (`mse_rollout_modular`, one launch per
rollout): each agent samples, scores and values its own preview, the flat action is stepped, and the reward is recorded
whole and in its sorting / pressing parts; `view()` hands a `PPOLearner` one agent's rows.  `ModularRolloutCollector`
is its multi-launch twin, the yardstick the kernel is tested against.
"""
from __future__ import annotations

from typing import Optional

import torch

from .batched import BatchedSortingEnv
from .policy import MlpPolicy


F32, I32, U8 = torch.float32, torch.int32, torch.uint8
ROW_DTYPES = {"observations": F32, "action_masks": U8, "actions": I32, "log_probs": F32, "values": F32, "rewards": F32,
              "episode_starts": U8, "last_values": F32, "last_dones": U8, "stepped_actions": I32, "expert_stepped": U8,
              "returns": F32, "expert_actions": I32}
POLICY_ROWS = ("observations", "action_masks", "actions", "log_probs", "values", "rewards", "episode_starts")


def rollout_buffers(env, K: int, last: bool = False, names=POLICY_ROWS, dims=None) -> dict:
    """The `MaskableRolloutBuffer`-shaped dict of device tensors every single-policy collector fills: `names` in that
    order, [K, N] each except `observations` [K, N, obs_dim], `action_masks` [K, N, n_actions] and the per-env rows
    `last_values` / `last_dones` [N], which last=True appends.  dims: (obs_dim, n_actions) when they are not the env's."""
    n, (obs_dim, n_actions) = env.num_envs, dims or (env.obs_dim, env.num_actions)
    shapes = {"observations": (K, n, obs_dim), "action_masks": (K, n, n_actions), "last_values": (n,), "last_dones": (n,)}
    names = tuple(names) + (("last_values", "last_dones") if last else ())
    return {k: torch.empty(shapes.get(k, (K, n)), dtype=ROW_DTYPES[k], device=env.device) for k in names}


def _check_policy_collector(env, policy, sort_policy, view: str = "own") -> None:
    """What `PolicyRolloutCollector` and `FusedPolicyRollout` refuse at construction."""
    if view not in ("own", "preview"):
        raise ValueError(f"view must be 'own' or 'preview', not {view!r}")
    if view == "preview" and env.kind != "mono":
        raise ValueError("view='preview' is the mono policy's in-step view of Env_3 (env_monolith.py:144-150): it needs a 'mono' env")
    if policy.obs_dim != env.obs_dim or policy.n_actions != env.num_actions:
        raise ValueError("policy dimensions do not match the env")
    if sort_policy is not None and (env.kind != "press" or sort_policy.obs_dim != 13 or sort_policy.n_actions != 2):
        raise ValueError("a sorting policy (13 -> 2) only applies to Env_2_Pressing")
    if not env.auto_reset:
        raise ValueError("collection needs auto_reset=True (episodes end inside a rollout)")


class _CollectorState:
    """The checkpoint surface of a collector (checkpoint.py): `KIND`, the `SEEDS` attributes, `n_steps` and the env's state
    dict; a collector that carries more between calls adds it in `_extra_state` and extends check / load."""

    KIND = None
    SEEDS = ("seed",)

    def _fingerprint(self) -> dict:
        return {"collector": self.KIND, **{k: getattr(self, k) for k in self.SEEDS}, "n_steps": self.n_steps}

    def _extra_state(self) -> dict:
        return {}

    def state_dict(self) -> dict:
        """`KIND` under "collector", the seeds, `n_steps`, what `_extra_state` adds, and the env's state dict."""
        return {**self._fingerprint(), **self._extra_state(), "env": self.env.state_dict()}

    def check_state_dict(self, sd: dict) -> None:
        """ValueError, with nothing touched, unless `sd` is this kind of collector's with these seeds and `n_steps` and
        the env accepts its part."""
        from .checkpoint import check_fingerprint

        mine = self._fingerprint()
        check_fingerprint({k: sd.get(k) for k in mine}, mine, type(self).__name__)
        if not isinstance(sd.get("env"), dict):
            raise ValueError(f"{type(self).__name__}: the checkpoint has no env state")
        self.env.check_state_dict(sd["env"])

    def load_state_dict(self, sd: dict) -> None:
        self.check_state_dict(sd)
        self.env.load_state_dict(sd["env"])  # refreshes env.obs / env.mask, which a stepwise collect() starts from


class _PolicyViewState(_CollectorState):
    """The single-policy collectors' checkpoint surface: _CollectorState's, plus the key `view` when it is "preview" (a
    checkpoint written before there was a view has none and is one of "own")."""

    view = "own"

    def _fingerprint(self) -> dict:
        return {**super()._fingerprint(), **({"view": self.view} if self.view == "preview" else {})}

    def check_state_dict(self, sd: dict) -> None:
        saved = sd.get("view", "own")
        if saved != self.view:
            raise ValueError(f"{type(self).__name__}: view mismatch: the checkpoint has {saved!r}, this collector {self.view!r}")
        super().check_state_dict(sd)


class PolicyRolloutCollector(_PolicyViewState):
    KIND = "two_launch"

    def __init__(self, env: BatchedSortingEnv, policy: MlpPolicy, n_steps: int, sort_policy: Optional[MlpPolicy] = None,
                 seed: int = 2024, expert_labels: bool = False, view: str = "own"):
        """view="preview" (a "mono" env): the policy is shown `env.mono_agent_obs()`, the observation after the step's flow
        update (Env_3_Monolith.step's stored mono_agent, env_monolith.py:144-150), and the bootstrap value comes from the
        final `mono_agent_obs()`; the row names are the same.  `FusedPolicyRollout(view="preview")`'s twin.
        expert_labels: `env.rule_actions()` of every state the rollout visits, taken before its step, is recorded in
        `buffers["expert_actions"]` (i32[K, N]): what the rule-based controller would do there, the labels of
        `PPOLearner(bc_coef=...)`.  The labels are outputs, not state: the checkpoint surface is the same."""
        _check_policy_collector(env, policy, sort_policy, view)
        self.env, self.policy, self.sort_policy, self.view = env, policy, sort_policy, view
        self.n_steps, self.seed, self.t = int(n_steps), int(seed), 0
        self.expert_labels = bool(expert_labels)
        self.buffers = rollout_buffers(env, self.n_steps, names=POLICY_ROWS + (("expert_actions",) if self.expert_labels else ()))
        self._last_done = torch.ones((env.num_envs,), dtype=torch.uint8, device=env.device)  # the envs were just reset
        self._out = None
        self._sort_out = None

    # ---- checkpoint: _CollectorState plus the policy stream's step `t` and the end marks of the last step (`_last_done`,
    # the next rollout's first `episode_starts`) -----------------------------------------------------------------------
    def _extra_state(self) -> dict:
        from .checkpoint import cpu

        return {"t": self.t, "last_done": cpu(self._last_done)}

    def check_state_dict(self, sd: dict) -> None:
        from .checkpoint import check_tensor

        super().check_state_dict(sd)
        check_tensor(sd, "last_done", self._last_done, "PolicyRolloutCollector")
        if isinstance(sd.get("t"), bool) or not isinstance(sd.get("t"), int) or sd["t"] < 0:
            raise ValueError(f"PolicyRolloutCollector: t must be a non-negative int, the checkpoint has {sd.get('t')!r}")

    def load_state_dict(self, sd: dict) -> None:
        super().load_state_dict(sd)
        self.t = sd["t"]
        self._last_done.copy_(sd["last_done"])

    def collect(self, deterministic: bool = False) -> dict:
        """K steps; returns the buffers plus `last_values` f32[N] (the bootstrap value of the state after the last
        step) and `last_dones`, as SB3's compute_returns_and_advantage wants them."""
        env, b = self.env, self.buffers
        preview = self.view == "preview"
        for k in range(self.n_steps):
            obs, mask = (env.mono_agent_obs() if preview else env.obs), env.mask
            b["observations"][k].copy_(obs)
            b["action_masks"][k].copy_(mask)
            b["episode_starts"][k].copy_(self._last_done)
            if self.expert_labels:
                b["expert_actions"][k].copy_(env.rule_actions())
            self._out = self.policy.forward(obs, mask, seed=self.seed, t=self.t, deterministic=deterministic,
                                            index_offset=env.index_offset, out=self._out)
            sort_mode = None
            if self.sort_policy is not None:
                self._sort_out = self.sort_policy.forward(env.sort_agent_obs(), None, deterministic=True, out=self._sort_out)
                sort_mode = self._sort_out["action"]
            b["actions"][k].copy_(self._out["action"])
            b["log_probs"][k].copy_(self._out["logp"])
            b["values"][k].copy_(self._out["value"])
            _, rew, done, _ = env.step(self._out["action"], sort_mode=sort_mode)
            b["rewards"][k].copy_(rew)
            self._last_done.copy_(done)
            self.t += 1
        last = self.policy.forward(env.mono_agent_obs() if preview else env.obs, env.mask, seed=self.seed, t=self.t, deterministic=True,
                                   index_offset=env.index_offset)
        return dict(b, last_values=last["value"], last_dones=self._last_done.clone())


class FusedPolicyRollout(_PolicyViewState):
    """K steps of policy forward + env transition per launch (`mse_rollout_policy`): MaskableRolloutBuffer-shaped
    device tensors [K, N, ...].  Env_2's sorting decisions: `sort_policy` (a 13 -> 2 MlpPolicy standing for the
    pre-trained sorting agent, evaluated inside the kernel), else `sort_mode` (a per-env tensor), else the reference's rule.
    Checkpoint: _CollectorState's alone - the kernel derives `episode_starts` from the env state and reads the step counter
    from the handle (`sort_mode`, a constructor argument, is given again at construction like the policies).
    view="preview" (a "mono" env): `collect()` is one `mse_rollout_policy_preview` launch at threshold 0 - the policy is shown
    the observation after the step's flow update, as the modular agents are; with expert_labels the same launch fills
    `expert_actions`.  `PolicyRolloutCollector(view="preview")`'s bits under the same row names."""

    KIND = "fused"

    def __init__(self, env: BatchedSortingEnv, policy: MlpPolicy, n_steps: int, seed: int = 2024,
                 sort_mode: Optional[torch.Tensor] = None, sort_policy: Optional[MlpPolicy] = None, expert_labels: bool = False,
                 view: str = "own"):
        """expert_labels: `collect()` is one `mse_rollout_policy_labelled` launch and the buffers gain `expert_actions`
        (i32[K, N]): the rule-based controller's action in every recorded state, `PolicyRolloutCollector(expert_labels=True)`'s
        bits.  The plain kernel runs at every size (no roles shape) and there is no in-loop sorting policy.  The labels are
        outputs, not state: the checkpoint surface is the same."""
        _check_policy_collector(env, policy, sort_policy, view)
        self.view = view
        if expert_labels and sort_policy is not None:
            raise ValueError("the one-launch labelled rollout has no in-loop sorting policy: collect with "
                             "PolicyRolloutCollector(sort_policy=..., expert_labels=True)")
        self.expert_labels = bool(expert_labels)
        self.env, self.policy, self.n_steps, self.seed = env, policy, int(n_steps), int(seed)
        self.sort_policy = sort_policy  # Env_2's pre-trained sorting agent, evaluated inside the kernel
        self.sort_mode = None if sort_mode is None else sort_mode.to(device=env.device, dtype=torch.int32).contiguous()
        self.buffers = rollout_buffers(env, self.n_steps, last=True,
                                       names=POLICY_ROWS + (("expert_actions",) if self.expert_labels else ()))

    def collect(self, n_steps: Optional[int] = None, deterministic: bool = False, use_action_masking: bool = True,
                check_overflow: bool = False) -> dict:
        """One launch.  n_steps <= the buffers' K (a shorter rollout fills the first rows).  The env's own obs / mask
        tensors are not refreshed (the state is; call env.refresh_outputs() to step it by hand afterwards)."""
        import ctypes as C

        from ._lib import MSE_STEP_CHECK_OVERFLOW, MSE_STEP_UNMASKED, check

        K = self.n_steps if n_steps is None else int(n_steps)
        if not 1 <= K <= self.n_steps:
            raise ValueError("n_steps must be in [1, the collector's K]")
        env, b = self.env, self.buffers
        flags = (0 if use_action_masking else MSE_STEP_UNMASKED) | (MSE_STEP_CHECK_OVERFLOW if check_overflow else 0)

        def ptr(x):
            return None if x is None else C.c_void_p(x.data_ptr())

        if self.view == "preview":
            from ._lib import MSE_PREVIEW_DETERMINISTIC, PREVIEW_BUFFER_NAMES, MsePreviewBuffers

            if not use_action_masking:
                raise ValueError("view='preview' predicts under the mask and applies the action unsanitised "
                                 "(env_monolith.py:148, :254-259): there is no use_action_masking=False")
            out = MsePreviewBuffers(C.sizeof(MsePreviewBuffers), 0,
                                    *(b[name].data_ptr() if name in b else None for name in PREVIEW_BUFFER_NAMES))
            pflags = (MSE_STEP_CHECK_OVERFLOW if check_overflow else 0) | (MSE_PREVIEW_DETERMINISTIC if deterministic else 0)
            with torch.cuda.device(env.device):  # threshold 0: the policy always steps; the mixture seed selects nothing
                check(env.L.mse_rollout_policy_preview(env._h, self.policy._h, K, self.seed, self.seed + 1, 0, pflags,
                                                       C.byref(out), env._stream()))
            return b
        if self.expert_labels:
            with torch.cuda.device(env.device):
                check(env.L.mse_rollout_policy_labelled(env._h, self.policy._h, K, self.seed, 1 if deterministic else 0,
                                                        ptr(self.sort_mode), flags, ptr(b["observations"]), ptr(b["action_masks"]),
                                                        ptr(b["actions"]), ptr(b["log_probs"]), ptr(b["values"]), ptr(b["rewards"]),
                                                        ptr(b["episode_starts"]), ptr(b["last_values"]), ptr(b["last_dones"]),
                                                        ptr(b["expert_actions"]), env._stream()))
            return b
        with torch.cuda.device(env.device):
            check(env.L.mse_rollout_policy(env._h, self.policy._h, None if self.sort_policy is None else self.sort_policy._h,
                                           K, self.seed, 1 if deterministic else 0,
                                           ptr(self.sort_mode), flags, ptr(b["observations"]), ptr(b["action_masks"]),
                                           ptr(b["actions"]), ptr(b["log_probs"]), ptr(b["values"]), ptr(b["rewards"]),
                                           ptr(b["episode_starts"]), ptr(b["last_values"]), ptr(b["last_dones"]),
                                           env._stream()))
        return b


class ModelRolloutCollector:
    """Env_3_Monolith.step(action=None, mode='model') for every env, one round of launches per step:
    mse_sort_agent_obs, mse_press_agent_obs, up to two deterministic MlpPolicy forwards (sort_agent 13 -> 2, press_agent
    16 -> 11), mse_model_actions drawing the parts no agent decides, mse_step.  press_agent_maskable: the pressing agent
    is a MaskablePPO, so with use_action_masking it is shown press_action_masks() (env_monolith.py:201-206).
    `collect` fills the buffers `BatchedSortingEnv.rollout(K, policy="model")` fills, with the same values."""

    def __init__(self, env: BatchedSortingEnv, sort_agent: Optional[MlpPolicy] = None,
                 press_agent: Optional[MlpPolicy] = None, press_agent_maskable: bool = True):
        if env.kind != "mono":
            raise ValueError("mode='model' exists on Env_3_Monolith only (env_monolith.py:186)")
        if sort_agent is not None and (sort_agent.obs_dim != 13 or sort_agent.n_actions != 2):
            raise ValueError("the sorting agent must be a 13 -> 2 policy")
        if press_agent is not None and (press_agent.obs_dim != 16 or press_agent.n_actions != 11):
            raise ValueError("the pressing agent must be a 16 -> 11 policy")
        if not env.auto_reset:
            raise ValueError("collection needs auto_reset=True (episodes end inside a rollout)")
        self.env, self.sort_agent, self.press_agent = env, sort_agent, press_agent
        self.press_agent_maskable = bool(press_agent_maskable)
        self._sort_out = self._press_out = None

    def collect(self, k_steps: int, use_action_masking: bool = True, check_overflow: bool = False,
                buffers: Optional[dict] = None) -> dict:
        env, K = self.env, int(k_steps)
        b = env.alloc_rollout(K, sort_obs=True, press_obs=True) if buffers is None else buffers
        masked_agent = self.press_agent is not None and use_action_masking and self.press_agent_maskable
        env.refresh_outputs()  # env.mask = action_masks() of the current state, whatever ran on the handle before
        for k in range(K):
            sort_obs, press_obs = env.sort_agent_obs(), env.press_agent_obs()
            if self.sort_agent is not None:
                self._sort_out = self.sort_agent.forward(sort_obs, None, deterministic=True, out=self._sort_out)
            if self.press_agent is not None:
                mask = env.mask[:, :11] if masked_agent else None  # press_action_masks()
                self._press_out = self.press_agent.forward(press_obs, mask, deterministic=True, out=self._press_out)
            action = env.model_actions(use_action_masking, draw_sort=self.sort_agent is None,
                                       draw_press=self.press_agent is None)
            if self.sort_agent is not None:
                action += 11 * self._sort_out["action"]
            if self.press_agent is not None:
                action += self._press_out["action"]
            # applied without sanitising (env_monolith.py:254-257): masked step semantics whatever use_action_masking
            obs, rew, done, mask = env.step(action, check_overflow=check_overflow)
            for key, v in (("actions", action), ("obs", obs), ("reward", rew), ("done", done), ("mask", mask),
                           ("sort_obs", sort_obs), ("press_obs", press_obs)):
                if b.get(key) is not None:
                    b[key][k].copy_(v)
        return b


# ---- the modular pair in the env it is deployed in (mse_rollout_modular) ----------------------------------------------
def _check_modular(env, sort_agent, press_agent, n_steps, sort_seed, press_seed) -> None:
    """What both modular collectors refuse before any handle is asked: the kernel's own argument rules."""
    if getattr(env, "kind", None) != "mono":
        raise ValueError("the modular rollout exists on Env_3_Monolith only")
    if sort_agent is None or press_agent is None:
        raise ValueError("both agents are required")
    if sort_agent.obs_dim != 13 or sort_agent.n_actions != 2:
        raise ValueError("the sorting agent must be a 13 -> 2 policy")
    if press_agent.obs_dim != 16 or press_agent.n_actions != 11:
        raise ValueError("the pressing agent must be a 16 -> 11 policy")
    if not env.auto_reset:
        raise ValueError("collection needs auto_reset=True (episodes end inside a rollout)")
    if int(n_steps) < 1:
        raise ValueError("n_steps must be >= 1")
    if int(sort_seed) == int(press_seed):
        raise ValueError("sort_seed == press_seed: the two agents would draw from one word")


def _modular_buffers(n: int, K: int, dev, parts: bool = True) -> dict:
    f32, i32, u8 = torch.float32, torch.int32, torch.uint8
    b = {
        "sort_obs": torch.empty((K, n, 13), dtype=f32, device=dev),
        "press_obs": torch.empty((K, n, 16), dtype=f32, device=dev),
        "press_masks": torch.empty((K, n, 11), dtype=u8, device=dev),
        "episode_starts": torch.empty((K, n), dtype=u8, device=dev),
        "sort_actions": torch.empty((K, n), dtype=i32, device=dev),
        "press_actions": torch.empty((K, n), dtype=i32, device=dev),
        "sort_log_probs": torch.empty((K, n), dtype=f32, device=dev),
        "press_log_probs": torch.empty((K, n), dtype=f32, device=dev),
        "sort_values": torch.empty((K, n), dtype=f32, device=dev),
        "press_values": torch.empty((K, n), dtype=f32, device=dev),
        "rewards": torch.empty((K, n), dtype=f32, device=dev),
        "sort_last_values": torch.empty((n,), dtype=f32, device=dev),
        "press_last_values": torch.empty((n,), dtype=f32, device=dev),
        "last_dones": torch.empty((n,), dtype=u8, device=dev),
    }
    if parts:
        b["rewards_sort"] = torch.empty((K, n), dtype=f32, device=dev)
        b["rewards_press"] = torch.empty((K, n), dtype=f32, device=dev)
    return b


def modular_view(buffers: dict, who: str, reward: str = "own", press_masked: bool = True) -> dict:
    """One agent's part of a modular collector's buffer dict under `PPOLearner`'s names; every value IS the buffer's
    tensor (no copy).  who: "sort" | "press".  reward: "own" - that agent's component (`rewards_sort` /
    `rewards_press`) - or "team", the sum both agents earned (`rewards`).  `action_masks` is None for the sorter, and for
    the presser when it was not shown its mask."""
    if who not in ("sort", "press"):
        raise ValueError(f"who must be 'sort' or 'press', not {who!r}")
    if reward not in ("own", "team"):
        raise ValueError(f"reward must be 'own' or 'team', not {reward!r}")
    rkey = "rewards" if reward == "team" else f"rewards_{who}"
    if buffers.get(rkey) is None:
        raise KeyError(f"this collector does not fill {rkey!r} (the multi-launch twin has no reward parts)")
    view = {
        "observations": buffers[f"{who}_obs"],
        "action_masks": buffers["press_masks"] if who == "press" and press_masked else None,
        "actions": buffers[f"{who}_actions"],
        "log_probs": buffers[f"{who}_log_probs"],
        "values": buffers[f"{who}_values"],
        "rewards": buffers[rkey],
        "episode_starts": buffers["episode_starts"],
        "last_values": buffers[f"{who}_last_values"],
        "last_dones": buffers["last_dones"],
    }
    if buffers.get(f"{who}_expert_actions") is not None:  # a labelled collector: that agent's half of the label
        view["expert_actions"] = buffers[f"{who}_expert_actions"]
    return view


def _modular_label_buffers(n: int, K: int, dev, returns: bool = False) -> dict:
    """What `expert_labels=True` adds to `_modular_buffers`: struct mse_modular_label_buffers' members, and `returns`
    with a `gamma`."""
    b = {"sort_expert_actions": torch.empty((K, n), dtype=I32, device=dev),
         "press_expert_actions": torch.empty((K, n), dtype=I32, device=dev),
         "stepped_actions": torch.empty((K, n), dtype=I32, device=dev),
         "expert_stepped": torch.empty((K, n), dtype=U8, device=dev)}
    if returns:
        b["returns"] = torch.empty((K, n), dtype=F32, device=dev)
    return b


def demo_view(buffers: dict, who: str, press_masked: bool = True) -> dict:
    """One agent's part of a LABELLED modular collector's buffer dict as `DemonstrationCollector(agent=who)`'s dict, what
    an `ImitationLearner` consumes; every value IS the buffer's tensor (no copy).  `actions` is that agent's half of the
    rule-based label, `rewards` the team reward, `returns` its discounted reward-to-go (None without a `gamma`);
    `action_masks` is None for the sorter, and for the presser when it was not shown its mask.  Buffers without labels
    are refused by name."""
    if who not in ("sort", "press"):
        raise ValueError(f"who must be 'sort' or 'press', not {who!r}")
    if buffers.get(f"{who}_expert_actions") is None:
        raise KeyError(f"demo_view: this collector does not fill '{who}_expert_actions' (construct it with expert_labels=True)")
    return {
        "observations": buffers[f"{who}_obs"],
        "action_masks": buffers["press_masks"] if who == "press" and press_masked else None,
        "actions": buffers[f"{who}_expert_actions"],
        "stepped_actions": buffers["stepped_actions"],
        "expert_stepped": buffers["expert_stepped"],
        "rewards": buffers["rewards"],
        "episode_starts": buffers["episode_starts"],
        "last_dones": buffers["last_dones"],
        "returns": buffers.get("returns"),
    }


def modular_mix_seed(sort_seed: int, press_seed: int, mix_seed: Optional[int] = None) -> int:
    """The seed of the who-steps stream of a labelled modular collector: `mix_seed`, or by default one past the larger agent
    seed.  A seed that is one of the agents' is refused: who steps and what that agent draws would come from one word."""
    mix = max(int(sort_seed), int(press_seed)) + 1 if mix_seed is None else int(mix_seed)
    if mix in (int(sort_seed), int(press_seed)):
        raise ValueError("mix_seed equals an agent's seed: who steps and what that agent draws would come from one word")
    return mix


class _ModularBase(_CollectorState):
    """Constructor and views the fused modular collector and its multi-launch twin share.  Checkpoint: _CollectorState's
    with both seeds - the kernel derives `episode_starts` from the env state, which also carries the policy step counter;
    a labelled collector adds `mix_seed` (checked like the seeds) and `beta` (restored).

    expert_labels=True: every recorded state also carries the rule-based controller's action in its two halves
    (`sort_expert_actions` = a // 11, `press_expert_actions` = a % 11; `view()` hands them to `PPOLearner(bc_coef=...)` as
    `expert_actions`), and per env and step the label is stepped with probability `beta`, else the agents' 11 sort + press
    (`stepped_actions`, `expert_stepped`): DAgger's mixture, decided by a word of `mix_seed`'s stream against
    `imitation.expert_threshold(beta)`; one decision covers both halves.  `beta` may be set between calls.  gamma: `collect()`
    also fills `returns`, the discounted reward-to-go of the team reward (`mse_gae` with zero values and lambda = 1,
    `DemonstrationCollector`'s definition).  `demo_view(who)` is what an `ImitationLearner` of that agent consumes."""

    KIND = "modular"
    SEEDS = ("sort_seed", "press_seed")
    PARTS = True  # fills rewards_sort / rewards_press

    def __init__(self, env: BatchedSortingEnv, sort_agent: MlpPolicy, press_agent: MlpPolicy, n_steps: int,
                 sort_seed: int = 2024, press_seed: int = 2025, press_masked: bool = True, expert_labels: bool = False,
                 beta: float = 0.0, mix_seed: Optional[int] = None, gamma: Optional[float] = None):
        _check_modular(env, sort_agent, press_agent, n_steps, sort_seed, press_seed)
        self.expert_labels = bool(expert_labels)
        if not self.expert_labels and (mix_seed is not None or gamma is not None):
            raise ValueError("mix_seed / gamma belong to the labelled rollout: they need expert_labels=True")
        self.env, self.sort_agent, self.press_agent = env, sort_agent, press_agent
        self.n_steps, self.sort_seed, self.press_seed = int(n_steps), int(sort_seed), int(press_seed)
        self.press_masked = bool(press_masked)
        self.mix_seed = modular_mix_seed(sort_seed, press_seed, mix_seed) if self.expert_labels else None
        self.gamma = None if gamma is None else float(gamma)
        self.beta = beta  # refuses NaN, values outside [0, 1], and anything but 0 without labels
        if self.expert_labels:
            self.SEEDS = type(self).SEEDS + ("mix_seed",)
        n, K, dev = env.num_envs, self.n_steps, env.device
        self.buffers = _modular_buffers(n, K, dev, self.PARTS)
        if self.expert_labels:
            self.buffers.update(_modular_label_buffers(n, K, dev, returns=self.gamma is not None))
        if self.gamma is not None:
            self._zeros = torch.zeros((K + 1, n), dtype=F32, device=dev)  # mse_gae's values and last_values
            self._adv = torch.empty((K, n), dtype=F32, device=dev)
        self._views: dict = {}

    @property
    def beta(self) -> float:
        return self._beta

    @beta.setter
    def beta(self, value: float) -> None:
        from .imitation import expert_threshold

        threshold = expert_threshold(value)
        if not self.expert_labels and threshold != 0:
            raise ValueError("beta != 0 needs expert_labels=True: without labels there is no expert to step")
        self._beta, self._threshold = float(value), threshold

    def view(self, who: str, reward: str = "own") -> dict:
        """`modular_view` of this collector's buffers.  The dict of a (who, reward) pair is kept, so the advantages and
        returns `compute_gae` adds to it are allocated once."""
        key = (who, reward)
        if key not in self._views:
            self._views[key] = modular_view(self.buffers, who, reward, self.press_masked)
        return self._views[key]

    def demo_view(self, who: str) -> dict:
        """`demo_view` of this collector's buffers (kept per agent); refused on a collector without labels."""
        if not self.expert_labels:
            raise ValueError("demo_view needs a collector constructed with expert_labels=True")
        key = (who, "demo")
        if key not in self._views:
            self._views[key] = demo_view(self.buffers, who, self.press_masked)
        return self._views[key]

    def _check_run(self, n_steps) -> int:
        K = self.n_steps if n_steps is None else int(n_steps)
        if not 1 <= K <= self.n_steps:
            raise ValueError("n_steps must be in [1, the collector's K]")
        return K

    def _fill_returns(self, K: int) -> None:
        """One `mse_gae` launch over the first K rows: zero values, lambda = 1, no bootstrap at the window's end."""
        import ctypes as C

        from ._lib import check

        env, b = self.env, self.buffers

        def ptr(x):
            return C.c_void_p(x.data_ptr())

        with torch.cuda.device(env.device):
            check(env.L.mse_gae(K, env.num_envs, ptr(b["rewards"]), ptr(self._zeros), ptr(b["episode_starts"]),
                                ptr(self._zeros[K]), ptr(b["last_dones"]), self.gamma, 1.0, ptr(self._adv), ptr(b["returns"]),
                                env._stream()))

    # ---- checkpoint: a labelled collector's who-steps stream and mixture ---------------------------------------------------
    def _extra_state(self) -> dict:
        return {"beta": self._beta} if self.expert_labels else {}

    def check_state_dict(self, sd: dict) -> None:
        super().check_state_dict(sd)
        if ("mix_seed" in sd) != self.expert_labels:
            raise ValueError(f"{type(self).__name__}: the checkpoint is of a collector "
                             f"{'with' if 'mix_seed' in sd else 'without'} expert labels, this one is "
                             f"{'with' if self.expert_labels else 'without'}")
        if self.expert_labels:
            from .imitation import expert_threshold

            if isinstance(sd.get("beta"), bool) or not isinstance(sd.get("beta"), (int, float)):
                raise ValueError(f"{type(self).__name__}: beta must be a number, the checkpoint has {sd.get('beta')!r}")
            expert_threshold(sd["beta"])

    def load_state_dict(self, sd: dict) -> None:
        super().load_state_dict(sd)
        if self.expert_labels:
            self.beta = sd["beta"]


class FusedModularRollout(_ModularBase):
    """The sorting agent (13 -> 2) and the pressing agent (16 -> 11) acting side by side in Env_3_Monolith, K steps per
    launch (`mse_rollout_modular`): per agent the rows a `PPOLearner` consumes - observations, actions,
    log-probabilities, values, the bootstrap value - plus the step's reward whole (`rewards`) and in its two parts
    (`rewards_sort`, `rewards_press`).  press_masked: the pressing agent is maskable and sees press_action_masks().
    expert_labels=True (see `_ModularBase`): `collect()` is one `mse_rollout_modular_labelled` launch - plus one `mse_gae`
    launch with a `gamma` - and at beta = 0 every other buffer holds the bits of the plain launch."""

    def collect(self, n_steps: Optional[int] = None, sort_deterministic: bool = False, press_deterministic: bool = False,
                check_overflow: bool = False) -> dict:
        """One launch.  n_steps <= the buffers' K (a shorter rollout fills the first rows).  The env's own obs / mask
        tensors are not refreshed (the state is; call env.refresh_outputs() to step it by hand afterwards)."""
        import ctypes as C

        from ._lib import (MODULAR_BUFFER_NAMES, MSE_MODEL_PRESS_AGENT_MASKED, MSE_MODULAR_PRESS_DETERMINISTIC,
                           MSE_MODULAR_SORT_DETERMINISTIC, MSE_STEP_CHECK_OVERFLOW, MseModularBuffers, check)

        K = self._check_run(n_steps)
        env, b = self.env, self.buffers
        flags = (MSE_MODEL_PRESS_AGENT_MASKED if self.press_masked else 0) | (MSE_STEP_CHECK_OVERFLOW if check_overflow else 0) | \
                (MSE_MODULAR_SORT_DETERMINISTIC if sort_deterministic else 0) | \
                (MSE_MODULAR_PRESS_DETERMINISTIC if press_deterministic else 0)
        out = MseModularBuffers(C.sizeof(MseModularBuffers), 0, *(b[name].data_ptr() for name in MODULAR_BUFFER_NAMES))
        if self.expert_labels:
            from ._lib import MODULAR_LABEL_BUFFER_NAMES, MseModularLabelBuffers

            labels = MseModularLabelBuffers(C.sizeof(MseModularLabelBuffers), 0,
                                            *(b[name].data_ptr() for name in MODULAR_LABEL_BUFFER_NAMES))
            with torch.cuda.device(env.device):
                check(env.L.mse_rollout_modular_labelled(env._h, self.sort_agent._h, self.press_agent._h, K, self.sort_seed,
                                                         self.press_seed, self.mix_seed, self._threshold, flags, C.byref(out),
                                                         C.byref(labels), env._stream()))
            if self.gamma is not None:
                self._fill_returns(K)
            return b
        with torch.cuda.device(env.device):
            check(env.L.mse_rollout_modular(env._h, self.sort_agent._h, self.press_agent._h, K, self.sort_seed,
                                            self.press_seed, flags, C.byref(out), env._stream()))
        return b


class ModularRolloutCollector(_ModularBase):
    """`FusedModularRollout`'s multi-launch twin, built from the sentence in include/mse.h that states what the kernel
    equals: per step mse_sort_agent_obs, mse_press_agent_obs, two `MlpPolicy.forward` calls (the two seeds, t = the
    handle's policy step counter, index_offset = the env's) and mse_step.  It fills every buffer except `rewards_sort` /
    `rewards_press` (mse_step does not return the parts).  The yardstick the kernel is held against, not a fallback: it
    refuses what the kernel refuses, by asking the library (`mse_rollout_modular_check`) at construction and before every
    collection.  Like the kernel it reads `episode_starts` off the env state, so it carries nothing between calls and
    its `state_dict` is the base class's."""

    KIND = "modular_twin"
    PARTS = False
    SNAP_CURRENT_STEP = 32  # column of mse_get_state's integer record that holds the env's current_step

    def __init__(self, env: BatchedSortingEnv, sort_agent: MlpPolicy, press_agent: MlpPolicy, n_steps: int,
                 sort_seed: int = 2024, press_seed: int = 2025, press_masked: bool = True, expert_labels: bool = False,
                 beta: float = 0.0, mix_seed: Optional[int] = None, gamma: Optional[float] = None):
        """expert_labels=True: per step also `env.rule_actions()` with its halves // 11 and % 11, the who-steps rule on the
        host (`mse_demo_who_steps_host`) and the step of the chosen flat action: `mse_rollout_modular_labelled`'s twin."""
        super().__init__(env, sort_agent, press_agent, n_steps, sort_seed, press_seed, press_masked, expert_labels, beta,
                         mix_seed, gamma)
        self._refusal(self.n_steps, 0)  # what the fused launch would refuse on this handle, with these agents
        self._last_done = torch.empty((env.num_envs,), dtype=torch.uint8, device=env.device)
        self._sort_out = self._press_out = None
        self._who_host = torch.empty((env.num_envs,), dtype=torch.uint8) if self.expert_labels else None

    def _refusal(self, K: int, flags: int) -> None:
        """Raises what `FusedModularRollout.collect` would raise for the same arguments (`mse_rollout_modular_check`, or
        `mse_rollout_modular_labelled_check` with labels: the kernel's own checks - the handle, the agents' form, an
        attached trace, tables that do not fit, the threshold and the mixture seed - and no launch)."""
        from ._lib import MSE_MODEL_PRESS_AGENT_MASKED, check

        env = self.env
        flags |= MSE_MODEL_PRESS_AGENT_MASKED if self.press_masked else 0
        if self.expert_labels:
            check(env.L.mse_rollout_modular_labelled_check(env._h, self.sort_agent._h, self.press_agent._h, K, self.sort_seed,
                                                           self.press_seed, self.mix_seed, self._threshold, flags))
            return
        check(env.L.mse_rollout_modular_check(env._h, self.sort_agent._h, self.press_agent._h, K, self.sort_seed,
                                              self.press_seed, flags))

    def _who_steps(self, t: int) -> torch.Tensor:
        """bool[N] on the device: the expert steps env j at step counter t (`mse_demo_who_steps_host`)."""
        import ctypes as C

        from ._lib import check

        env, w = self.env, self._who_host
        check(env.L.mse_demo_who_steps_host(env.num_envs, env.index_offset, self.mix_seed, int(t), self._threshold,
                                            C.c_void_p(w.data_ptr())))
        return w.to(env.device).bool()

    def collect(self, n_steps: Optional[int] = None, sort_deterministic: bool = False, press_deterministic: bool = False,
                check_overflow: bool = False) -> dict:
        from ._lib import MSE_STEP_CHECK_OVERFLOW

        K = self._check_run(n_steps)
        env, b = self.env, self.buffers
        self._refusal(K, MSE_STEP_CHECK_OVERFLOW if check_overflow else 0)
        env.refresh_outputs()  # env.mask = action_masks() of the current state, whatever ran on the handle before
        # the first row's episode starts come from the state, as the kernel takes them (current_step == 0): nothing is
        # carried between calls, so a restored or hand-stepped handle gives the rows the kernel gives
        self._last_done.copy_(env.get_state()[0][:, self.SNAP_CURRENT_STEP] == 0)
        for k in range(K):
            sort_obs, press_obs = env.sort_agent_obs(), env.press_agent_obs()
            press_mask = env.mask[:, :11]  # press_action_masks()
            t = env.policy_step
            self._sort_out = self.sort_agent.forward(sort_obs, None, seed=self.sort_seed, t=t, deterministic=sort_deterministic,
                                                     index_offset=env.index_offset, out=self._sort_out)
            self._press_out = self.press_agent.forward(press_obs, press_mask if self.press_masked else None,
                                                       seed=self.press_seed, t=t, deterministic=press_deterministic,
                                                       index_offset=env.index_offset, out=self._press_out)
            b["sort_obs"][k].copy_(sort_obs)
            b["press_obs"][k].copy_(press_obs)
            b["press_masks"][k].copy_(press_mask)
            b["episode_starts"][k].copy_(self._last_done)
            for who, o in (("sort", self._sort_out), ("press", self._press_out)):
                b[f"{who}_actions"][k].copy_(o["action"])
                b[f"{who}_log_probs"][k].copy_(o["logp"])
                b[f"{who}_values"][k].copy_(o["value"])
            action = 11 * self._sort_out["action"] + self._press_out["action"]
            if self.expert_labels:
                rule = env.rule_actions()  # of the state the rows show; no stream is read
                who = self._who_steps(t)
                action = torch.where(who, rule, action)
                b["sort_expert_actions"][k].copy_(rule // 11)
                b["press_expert_actions"][k].copy_(rule % 11)
                b["stepped_actions"][k].copy_(action)
                b["expert_stepped"][k].copy_(who)
            # applied without sanitising (env_monolith.py:254-257): the masked step
            _, rew, done, _ = env.step(action, check_overflow=check_overflow)
            b["rewards"][k].copy_(rew)
            self._last_done.copy_(done)
        t = env.policy_step
        last_s = self.sort_agent.forward(env.sort_agent_obs(), None, seed=self.sort_seed, t=t, deterministic=True,
                                         index_offset=env.index_offset)
        last_p = self.press_agent.forward(env.press_agent_obs(), None, seed=self.press_seed, t=t, deterministic=True,
                                          index_offset=env.index_offset)
        b["sort_last_values"].copy_(last_s["value"])
        b["press_last_values"].copy_(last_p["value"])
        b["last_dones"].copy_(self._last_done)
        if self.gamma is not None:
            self._fill_returns(K)
        return b
