"""Torch-native batched front-end of the HIP step engine: N env instances, one per GPU lane.

This is the zero-host-copy surface (`step(actions) -> (obs, reward, done, mask)` on device tensors)
that the single-env Gymnasium views (envs.py) and the SB3 VecEnv adapter (vec_env.py) sit on.
PyTorch is plumbing here: device memory for the I/O buffers and the HIP stream; every transition
is computed by libmse_hip.so through the C ABI of include/mse.h.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib
from ._lib import (MSE_MODEL_NO_PRESS_DRAW, MSE_MODEL_NO_SORT_DRAW, MSE_MODEL_PRESS_AGENT_MASKED, MSE_ROLLOUT_RULE_BASED, MSE_SNAP_INTS, MSE_SNAP_RNG_WORDS,
                   MSE_STEP_CHECK_OVERFLOW, MSE_STEP_SANITIZE_LATE, MSE_STEP_UNMASKED, MSE_TRACE_COLS, check, load_library)
from .config import NUM_ACTIONS, OBS_DIM, SortingEnvConfig


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


LOOKAHEAD_BASES = ("random", "rule_based")  # mse_lookahead's base_policy codes 0 and 1; 2 is the network (mse_lookahead_net)


def lookahead_network(base_policy, leaf_value):
    """(network or None, base_policy code) of a lookahead call.  base_policy: one of the two strings or a policy object
    (`MlpPolicy`); leaf_value: None or a policy object.  The kernel holds one weight image, so two different objects for
    base and leaf are a ValueError."""
    if isinstance(base_policy, str):
        if base_policy not in LOOKAHEAD_BASES:
            raise ValueError(f"base_policy must be 'rule_based' or 'random', not {base_policy!r}")
        base_net, code = None, LOOKAHEAD_BASES.index(base_policy)
    elif base_policy is None or not all(hasattr(base_policy, k) for k in ("obs_dim", "n_actions")):
        raise ValueError(f"base_policy must be 'rule_based', 'random' or an MlpPolicy, not {base_policy!r}")
    else:
        base_net, code = base_policy, 2
    if leaf_value is not None and not all(hasattr(leaf_value, k) for k in ("obs_dim", "n_actions")):
        raise ValueError(f"leaf_value must be None or an MlpPolicy, not {leaf_value!r}")
    if base_net is not None and leaf_value is not None and base_net is not leaf_value:
        raise ValueError("base_policy and leaf_value must be the same MlpPolicy object: the lookahead kernel holds one weight image")
    return (base_net if base_net is not None else leaf_value), code


def _other_device(a, b) -> bool:
    a, b = torch.device(a), torch.device(b)
    return a.type != b.type or (a.index is not None and b.index is not None and a.index != b.index)


class BatchedSortingEnv:
    """N independent Env_1_Sorting / Env_2_Pressing / Env_3_Monolith instances on one MI355X.

    kind: "sort" | "press" | "mono" (the reference's env.name values).
    Env i is seeded like the reference's `Env(seed=base_seed + index_offset + i)` followed by
    `reset(seed=...)`: results do not depend on how envs are sharded over GPUs.
    """

    def __init__(self, kind: str = "mono", num_envs: int = 1, device: int | str | torch.device = 0,
                 base_seed: int = 0, seeds: Optional[torch.Tensor] = None, max_steps: int = 50,
                 noise_sorting: Optional[float] = 0.05, balesize: Optional[int] = 200,
                 config: Optional[SortingEnvConfig] = None, auto_reset: bool = True,
                 track_bales: bool = True, literal_choice: bool = False, index_offset: int = 0,
                 reset_now: bool = True, rollout_pipeline: int = 0, library: Optional[str] = None):
        if kind not in OBS_DIM:
            raise ValueError(f"kind must be one of {sorted(OBS_DIM)}")
        if not torch.cuda.is_available():
            raise RuntimeError("BatchedSortingEnv needs a HIP device: the step path has no CPU fallback")
        self.L = load_library(library)  # `library`: another build of the same source (tests)
        self.kind = self.name = kind
        self.num_envs = int(num_envs)
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self.config = config if config is not None else SortingEnvConfig()
        self.max_steps = int(max_steps)
        self.index_offset = int(index_offset)
        self.obs_dim, self.num_actions = OBS_DIM[kind], NUM_ACTIONS[kind]
        self._cfg_struct = self.config.to_struct(kind, max_steps, noise_sorting, balesize, auto_reset,
                                                 track_bales, literal_choice, rollout_pipeline)
        self.auto_reset = bool(auto_reset)
        h = C.c_void_p()
        dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        check(self.L.mse_create_indexed(C.byref(h), C.byref(self._cfg_struct), self.num_envs, dev_index,
                                        self.index_offset))
        self._h = h
        self._trace_buf, self._trace_n = None, 0
        n, dev = self.num_envs, self.device
        self.obs = torch.zeros((n, self.obs_dim), dtype=torch.float32, device=dev)
        self.reward = torch.zeros((n,), dtype=torch.float32, device=dev)
        self.reward64 = torch.zeros((n,), dtype=torch.float64, device=dev)
        self.done = torch.zeros((n,), dtype=torch.uint8, device=dev)
        self.mask = torch.zeros((n, self.num_actions), dtype=torch.uint8, device=dev)
        self.terminal_obs = torch.zeros((n, self.obs_dim), dtype=torch.float32, device=dev)
        if seeds is None:
            seeds = (torch.arange(n, dtype=torch.int64, device=dev) + (int(base_seed) + self.index_offset))
        self.seeds = seeds.to(device=dev, dtype=torch.int64).contiguous()
        if reset_now:
            self.reset(seeds=self.seeds)

    # ---- lifecycle -------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self.L.mse_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # ---- reference surface, batched ----------------------------------------------------------
    def reset(self, seeds: Optional[torch.Tensor] = None, which: Optional[torch.Tensor] = None):
        """reset(seed=seeds[i]) for every env (or those with which[i] != 0); seeds=None is the
        reference's reset(seed=None): streams continue.  Returns (obs, mask) device tensors."""
        if seeds is not None:
            seeds = seeds.to(device=self.device, dtype=torch.int64).contiguous()
            if seeds.numel() != self.num_envs:
                raise ValueError("seeds must have one entry per env")
            if bool((seeds < 0).any()):
                raise ValueError("seeds must be non-negative")  # np.random.default_rng rejects negatives
        if which is not None:
            which = which.to(device=self.device, dtype=torch.uint8).contiguous()
        with torch.cuda.device(self.device):
            check(self.L.mse_reset(self._h, _ptr(seeds), _ptr(which), _ptr(self.obs), _ptr(self.mask), self._stream()))
        return self.obs, self.mask

    def step(self, actions: torch.Tensor, sort_mode: Optional[torch.Tensor] = None,
             use_action_masking: bool = True, check_overflow: bool = False, want_reward64: bool = False,
             want_terminal_obs: bool = False, sanitize_late: bool = False):
        """One transition of all N envs.  Returns (obs, reward, done, mask): views of buffers that
        the next step overwrites.  sanitize_late (Env_3 without masking): validate the press action after
        sort_material, as the reference's mode='random' does (MSE_STEP_SANITIZE_LATE)."""
        if actions.dtype != torch.int32 or not actions.is_contiguous() or actions.device != self.device:
            actions = actions.to(device=self.device, dtype=torch.int32).contiguous()
        if actions.numel() != self.num_envs:
            raise ValueError("actions must have one entry per env")
        if sort_mode is not None:
            sort_mode = sort_mode.to(device=self.device, dtype=torch.int32).contiguous()
        flags = (0 if use_action_masking else MSE_STEP_UNMASKED) | (MSE_STEP_CHECK_OVERFLOW if check_overflow else 0) | \
                (MSE_STEP_SANITIZE_LATE if sanitize_late else 0)
        with torch.cuda.device(self.device):
            check(self.L.mse_step(self._h, _ptr(actions), _ptr(sort_mode), flags, _ptr(self.obs), _ptr(self.reward),
                                  _ptr(self.reward64) if want_reward64 else None, _ptr(self.done), _ptr(self.mask),
                                  _ptr(self.terminal_obs) if want_terminal_obs else None, self._stream()))
        if self._trace_buf is not None:
            self._trace_n += 1
        return self.obs, self.reward, self.done, self.mask

    def action_masks(self) -> torch.Tensor:
        out = torch.empty((self.num_envs, self.num_actions), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            check(self.L.mse_action_masks(self._h, _ptr(out), self._stream()))
        return out

    def sort_agent_obs(self) -> torch.Tensor:
        """f32[N, 13]: what Env_2_Pressing.step hands its sorting agent on the coming step (env_2_press.py:101):
        get_sort_obs() after that step's flow update.  Feed the agent's decisions back as step(..., sort_mode=)."""
        out = torch.empty((self.num_envs, 13), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            check(self.L.mse_sort_agent_obs(self._h, _ptr(out), self._stream()))
        return out

    def press_agent_obs(self) -> torch.Tensor:
        """f32[N, 16]: get_press_obs() after the coming step's flow update - what Env_3_Monolith.step(mode='model')
        hands its press_agent (env_monolith.py:198-210)."""
        out = torch.empty((self.num_envs, 16), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            check(self.L.mse_press_agent_obs(self._h, _ptr(out), self._stream()))
        return out

    def mono_agent_obs(self) -> torch.Tensor:
        """f32[N, 29]: what Env_3_Monolith.step hands a stored mono_agent (env_monolith.py:144-150): get_obs() after the
        coming step's flow update, `sort_agent_obs()` || `press_agent_obs()` on bits, in one launch.  Env_3 only."""
        out = torch.empty((self.num_envs, 29), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            check(self.L.mse_mono_agent_obs(self._h, _ptr(out), self._stream()))
        return out

    def sample_actions(self, policy_seed: int = 2024) -> torch.Tensor:
        out = torch.empty((self.num_envs,), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            check(self.L.mse_sample_actions(self._h, int(policy_seed), _ptr(out), self._stream()))
        return out

    def rule_actions(self) -> torch.Tensor:
        """The reference's rule-based policy (mode='rule_based') evaluated on the device."""
        out = torch.empty((self.num_envs,), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            check(self.L.mse_rule_actions(self._h, _ptr(out), self._stream()))
        return out

    def model_actions(self, use_action_masking: bool = True, draw_sort: bool = True, draw_press: bool = True) -> torch.Tensor:
        """Env_3_Monolith.step(mode='model') with no agents assigned (env_monolith.py:186-221): the env's own
        rng_sorting / rng_pressing draws, NumPy-exact; the streams drawn from advance (draw_sort / draw_press = False:
        an assigned agent decides that part, it comes back as 0).  Step the result with masking semantics."""
        out = torch.empty((self.num_envs,), dtype=torch.int32, device=self.device)
        flags = (0 if use_action_masking else MSE_STEP_UNMASKED) | (0 if draw_sort else MSE_MODEL_NO_SORT_DRAW) | \
                (0 if draw_press else MSE_MODEL_NO_PRESS_DRAW)
        with torch.cuda.device(self.device):
            check(self.L.mse_model_actions(self._h, flags, _ptr(out), self._stream()))
        return out

    # ---- opt-in trace of one env, or of all (the reference's dashboard ledgers) ------------------------
    def trace_begin(self, env_index: int = 0, capacity: int = 4096) -> None:
        """From now on every step() appends one record f64[MSE_TRACE_COLS] for env `env_index` (mse_trace_begin)."""
        self._trace_buf = torch.zeros((int(capacity), MSE_TRACE_COLS), dtype=torch.float64, device=self.device)
        self._trace_n = 0
        check(self.L.mse_trace_begin(self._h, int(env_index), _ptr(self._trace_buf), int(capacity)))

    def trace_begin_all(self, capacity: int) -> None:
        """From now on every step() stores the record of EVERY env (mse_trace_begin_all): `trace_records()` is then
        f64[n, MSE_TRACE_COLS, N], one plane of N doubles per column per step - what `PlantStats.update` scans and
        `EnvTrace.from_records` reads.  capacity x 320 x N bytes of device memory; a buffer of the same capacity is
        used again by the next call (records handed out earlier are views of it)."""
        shape = (int(capacity), MSE_TRACE_COLS, self.num_envs)
        buf = getattr(self, "_trace_all_buf", None)
        if buf is None or tuple(buf.shape) != shape:
            buf = self._trace_all_buf = torch.zeros(shape, dtype=torch.float64, device=self.device)
        check(self.L.mse_trace_begin_all(self._h, _ptr(buf), int(capacity)))
        self._trace_buf, self._trace_n = buf, 0

    def trace_records(self) -> torch.Tensor:
        """The records written so far (synchronises the stream); the trace stays attached."""
        if getattr(self, "_trace_buf", None) is None:
            return torch.zeros((0, MSE_TRACE_COLS), dtype=torch.float64, device=self.device)
        torch.cuda.current_stream(self.device).synchronize()
        return self._trace_buf[: self._trace_n]

    def trace_end(self) -> torch.Tensor:
        """Detaches the trace (of either kind) and returns its records, f64[n, MSE_TRACE_COLS] or f64[n, MSE_TRACE_COLS, N]."""
        rec = self.trace_records().clone()
        check(self.L.mse_trace_end(self._h, None))
        self._trace_buf = None
        return rec

    # ---- policy-stream counter (host-side handle state, see include/mse.h) ---------------------------
    @property
    def policy_step(self) -> int:
        v = C.c_uint64(0)
        check(self.L.mse_get_policy_step(self._h, C.byref(v)))
        return int(v.value)

    @policy_step.setter
    def policy_step(self, t: int) -> None:
        check(self.L.mse_set_policy_step(self._h, int(t)))

    def alloc_rollout(self, k_steps: int, obs=True, mask=True, actions=True, reward=True, done=True,
                      sort_obs=False, press_obs=False):
        """Step-major rollout buffers.  sort_obs / press_obs (policy="model"): the agents' views of every step,
        f32[K, N, 13] / f32[K, N, 16], under keys that are only there when asked for."""
        n, dev, K = self.num_envs, self.device, int(k_steps)
        buffers = {
            "actions": torch.empty((K, n), dtype=torch.int32, device=dev) if actions else None,
            "obs": torch.empty((K, n, self.obs_dim), dtype=torch.float32, device=dev) if obs else None,
            "reward": torch.empty((K, n), dtype=torch.float32, device=dev) if reward else None,
            "done": torch.empty((K, n), dtype=torch.uint8, device=dev) if done else None,
            "mask": torch.empty((K, n, self.num_actions), dtype=torch.uint8, device=dev) if mask else None,
        }
        if sort_obs:
            buffers["sort_obs"] = torch.empty((K, n, 13), dtype=torch.float32, device=dev)
        if press_obs:
            buffers["press_obs"] = torch.empty((K, n, 16), dtype=torch.float32, device=dev)
        return buffers

    def rollout(self, k_steps: int, policy_seed: int = 2024, buffers: Optional[dict] = None,
                sort_mode: Optional[torch.Tensor] = None, use_action_masking: bool = True,
                check_overflow: bool = False, policy: str = "random", sort_agent=None, press_agent=None,
                press_agent_maskable: bool = True) -> dict:
        """K fused steps in one kernel launch under an on-device policy: "random" (masked-uniform),
        "rule_based" (the reference's mode='rule_based') or, on Env_3, "model": Env_3_Monolith.step(action=None,
        mode='model') (env_monolith.py:186-221) with an optional sorting agent (MlpPolicy 13 -> 2) and pressing agent
        (MlpPolicy 16 -> 11) evaluated inside the kernel (argmax), the env's own rng_sorting / rng_pressing drawing
        the part no agent decides (mse_rollout_model).  press_agent_maskable: the pressing agent is a MaskablePPO, so
        with use_action_masking it is shown press_action_masks() (env_monolith.py:201-206)."""
        if policy == "model":
            if sort_mode is not None:
                raise ValueError("policy='model' takes its sorting decisions from sort_agent or rng_sorting, not sort_mode")
            return self._rollout_model(k_steps, buffers, use_action_masking, check_overflow, sort_agent, press_agent,
                                       press_agent_maskable)
        if buffers is None:
            buffers = self.alloc_rollout(k_steps)
        if sort_mode is not None:
            sort_mode = sort_mode.to(device=self.device, dtype=torch.int32).contiguous()
        flags = (0 if use_action_masking else MSE_STEP_UNMASKED) | (MSE_STEP_CHECK_OVERFLOW if check_overflow else 0)
        if not use_action_masking and self.kind == "mono" and policy == "random":
            flags |= MSE_STEP_SANITIZE_LATE  # the reference's mode='random' sequencing (env_monolith.py:245-253)
        if policy == "rule_based":
            flags |= MSE_ROLLOUT_RULE_BASED
        elif policy != "random":
            raise ValueError("policy must be 'random', 'rule_based' or 'model'")
        with torch.cuda.device(self.device):
            check(self.L.mse_rollout(self._h, int(k_steps), int(policy_seed), _ptr(sort_mode), flags,
                                     _ptr(buffers.get("actions")), _ptr(buffers.get("obs")),
                                     _ptr(buffers.get("reward")), _ptr(buffers.get("done")),
                                     _ptr(buffers.get("mask")), self._stream()))
        return buffers

    def _rollout_model(self, k_steps, buffers, use_action_masking, check_overflow, sort_agent, press_agent,
                       press_agent_maskable):
        if buffers is None:
            buffers = self.alloc_rollout(k_steps, sort_obs=True, press_obs=True)
        for key, b in buffers.items():  # the kernel writes K full rows into every buffer it is given
            if b is not None and (b.shape[0] < int(k_steps) or b.shape[1] != self.num_envs or not b.is_contiguous()):
                raise ValueError(f"buffers[{key!r}] must be a contiguous [>= {int(k_steps)}, {self.num_envs}, ...] tensor")
        flags = (0 if use_action_masking else MSE_STEP_UNMASKED) | (MSE_STEP_CHECK_OVERFLOW if check_overflow else 0)
        if press_agent is not None and use_action_masking and press_agent_maskable:
            flags |= MSE_MODEL_PRESS_AGENT_MASKED
        with torch.cuda.device(self.device):
            check(self.L.mse_rollout_model(self._h, None if sort_agent is None else sort_agent._h,
                                           None if press_agent is None else press_agent._h, int(k_steps), flags,
                                           _ptr(buffers.get("actions")), _ptr(buffers.get("obs")),
                                           _ptr(buffers.get("reward")), _ptr(buffers.get("done")),
                                           _ptr(buffers.get("mask")), _ptr(buffers.get("sort_obs")),
                                           _ptr(buffers.get("press_obs")), self._stream()))
        return buffers

    # ---- lookahead: every env forked once per candidate action and sample, in one launch (mse_lookahead) ---------------
    def lookahead(self, horizon: int, gamma: float = 1.0, base_policy="rule_based", streams: str = "fresh", seed: int = 0,
                  base_seed: int = 2024, n_samples: int = 1, sort_mode: Optional[torch.Tensor] = None,
                  check_overflow: bool = False, out: Optional[dict] = None, leaf_value=None,
                  base_deterministic: bool = True) -> dict:
        """The rollout algorithm's inner loop in one `mse_lookahead` call, no host copy: per env, every action is tried on a
        copy of the env's current state and followed by horizon - 1 steps of `base_policy` ("rule_based" | "random", the
        latter drawn with `base_seed`); q[a, i] is the mean discounted return over `n_samples` forks, -inf where
        `action_masks()` forbids a; `action` the legal candidate of largest q (ties: the lowest), `value` its q.
        streams="fresh": sample m of env i draws from the streams of `reset(seed=mse_lookahead_stream_seed(seed,
        index_offset + i, m))`; streams="own": the fork continues the env's own streams (clairvoyant).  The env is not
        touched.  Returns {"q": f64[A, N], "action": i32[N], "value": f64[N]}; out: the dict of an earlier call, written again
        and returned (the workspace is kept by the env and grows with n_samples).  include/mse.h has the full contract;
        `lookahead.lookahead_reference` is the multi-launch twin.
        With a network (`mse_lookahead_net`): base_policy may be an `MlpPolicy` - steps 1 .. horizon - 1 take its
        `forward(obs, mask, seed=base_seed, t=s)` action, the argmax with base_deterministic (the default), a sample
        otherwise -, and leaf_value an `MlpPolicy` whose critic's value of the state a fork stands in after `horizon` steps
        is added with the running discount unless the fork's episode ended.  The kernel holds one weight image: base and
        leaf must be the same object.  The handle is live: every call plans with the policy's current weights."""
        net, base_code = lookahead_network(base_policy, leaf_value)
        if net is not None and (net.obs_dim != self.obs_dim or net.n_actions != self.num_actions or
                                _other_device(net.device, self.device)):
            raise ValueError(f"the lookahead's network must be a {self.obs_dim} -> {self.num_actions} policy on {self.device}")
        if streams not in ("fresh", "own"):
            raise ValueError(f"streams must be 'fresh' or 'own', not {streams!r}")
        if int(horizon) < 1:
            raise ValueError("horizon must be >= 1")
        if int(n_samples) < 1:
            raise ValueError("n_samples must be >= 1")
        if sort_mode is not None:
            sort_mode = sort_mode.to(device=self.device, dtype=torch.int32).contiguous()
            if sort_mode.numel() != self.num_envs:
                raise ValueError("sort_mode must have one entry per env")
        n, A, dev = self.num_envs, self.num_actions, self.device
        need = int(self.L.mse_lookahead_workspace_bytes(self._h, int(n_samples)))
        if need < 0:
            check(need)
        ws = getattr(self, "_lookahead_ws", None)
        if ws is None or ws.numel() < need:
            ws = self._lookahead_ws = torch.empty((need,), dtype=torch.uint8, device=dev)
        if out is None:
            out = {"q": torch.empty((A, n), dtype=torch.float64, device=dev), "action": torch.empty((n,), dtype=torch.int32, device=dev),
                   "value": torch.empty((n,), dtype=torch.float64, device=dev)}
        for key, shape, dt in (("q", (A, n), torch.float64), ("action", (n,), torch.int32), ("value", (n,), torch.float64)):
            t = out.get(key)
            if t is None or t.dtype != dt or t.device != dev or not t.is_contiguous() or tuple(t.shape) != shape:
                raise ValueError(f"out[{key!r}] must be a contiguous {dt} device tensor of shape {shape}")
        flags = MSE_STEP_CHECK_OVERFLOW if check_overflow else 0
        with torch.cuda.device(self.device):
            if net is None:
                check(self.L.mse_lookahead(self._h, int(horizon), float(gamma), base_code, int(base_seed),
                                           1 if streams == "fresh" else 0, int(seed), int(n_samples), _ptr(sort_mode), flags,
                                           _ptr(out["q"]), _ptr(out["action"]), _ptr(out["value"]), _ptr(ws), self._stream()))
            else:
                check(self.L.mse_lookahead_net(self._h, net._h, int(horizon), float(gamma), base_code,
                                               1 if base_deterministic else 0, int(base_seed), 0 if leaf_value is None else 1,
                                               1 if streams == "fresh" else 0, int(seed), int(n_samples), _ptr(sort_mode), flags,
                                               _ptr(out["q"]), _ptr(out["action"]), _ptr(out["value"]), _ptr(ws), self._stream()))
        return out

    # ---- state export / import (tests, checkpoint, dashboard trace) ---------------------------
    def get_state(self):
        n, dev = self.num_envs, self.device
        ints = torch.empty((n, MSE_SNAP_INTS), dtype=torch.int64, device=dev)
        dbls = torch.empty((n, 4), dtype=torch.float64, device=dev)
        rng = torch.empty((n, MSE_SNAP_RNG_WORDS), dtype=torch.int64, device=dev)  # raw u64 words
        with torch.cuda.device(self.device):
            check(self.L.mse_get_state(self._h, _ptr(ints), _ptr(dbls), _ptr(rng), self._stream()))
        return ints, dbls, rng

    def set_state(self, ints=None, dbls=None, rng=None):
        def prep(t, dt):
            return None if t is None else t.to(device=self.device, dtype=dt).contiguous()
        ints, dbls, rng = prep(ints, torch.int64), prep(dbls, torch.float64), prep(rng, torch.int64)
        with torch.cuda.device(self.device):
            check(self.L.mse_set_state(self._h, _ptr(ints), _ptr(dbls), _ptr(rng), self._stream()))

    def refresh_outputs(self):
        """Rewrites self.obs / self.mask from the current state (after set_state): a reset that resets no env."""
        none = torch.zeros((self.num_envs,), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            check(self.L.mse_reset(self._h, None, _ptr(none), _ptr(self.obs), _ptr(self.mask), self._stream()))
        return self.obs, self.mask

    # ---- checkpoint (checkpoint.py) ------------------------------------------------------------------------------------
    def fingerprint(self) -> dict:
        """What must be equal for a state record to mean the same thing on another handle: `kind`, `num_envs`,
        `max_steps`, `index_offset`, `auto_reset` and the bytes of the compiled config struct (u8 tensor)."""
        cfg = torch.frombuffer(bytearray(bytes(self._cfg_struct)), dtype=torch.uint8).clone()
        return {"kind": self.kind, "num_envs": self.num_envs, "max_steps": self.max_steps, "index_offset": self.index_offset,
                "auto_reset": self.auto_reset, "config": cfg}

    def _refuse_trace(self, what: str) -> None:
        if self._trace_buf is not None:
            raise RuntimeError(f"{what} with a trace attached: the trace's step count is not part of the state (trace_end() first)")

    def state_dict(self) -> dict:
        """CPU copies of the three `get_state()` tensors, `policy_step`, `seeds` and the `fingerprint()`.  `reward`,
        `done` and `terminal_obs` of the last step are outputs, not state, and are not saved; `obs` and `mask` are
        functions of the state (`refresh_outputs`).  Refused while a trace is attached."""
        from .checkpoint import cpu

        self._refuse_trace("state_dict()")
        ints, dbls, rng = self.get_state()
        return {"ints": cpu(ints), "dbls": cpu(dbls), "rng": cpu(rng), "policy_step": self.policy_step,
                "seeds": cpu(self.seeds), "fingerprint": self.fingerprint()}

    def check_state_dict(self, sd: dict) -> None:
        """ValueError naming every differing fingerprint field (a differing config struct by its members, as
        `config.<member>`), or a tensor of the wrong shape; nothing is touched."""
        from .checkpoint import check_tensor, diff_fields, mismatch_message

        self._refuse_trace("load_state_dict()")
        saved, mine = dict(sd.get("fingerprint") or {}), self.fingerprint()
        diffs = diff_fields(saved, mine)
        at = [i for i, d in enumerate(diffs) if d[0] == "config"]
        if at and isinstance(saved.get("config"), torch.Tensor) and saved["config"].numel() == mine["config"].numel():
            theirs = _lib.MseConfigStruct.from_buffer_copy(bytes(saved["config"].to(torch.uint8).tolist()))

            def plain(v):
                return [plain(x) for x in v] if hasattr(v, "__len__") else v

            members = [(f"config.{name}", plain(getattr(theirs, name)), plain(getattr(self._cfg_struct, name)))
                       for name, *_ in _lib.MseConfigStruct._fields_]
            members = [m for m in members if m[1] != m[2]]
            if members:
                diffs[at[0]:at[0] + 1] = members
        if diffs:
            raise ValueError(mismatch_message(f"BatchedSortingEnv({self.kind!r}, num_envs={self.num_envs})", diffs))
        n = self.num_envs
        for key, like in (("ints", torch.empty((n, MSE_SNAP_INTS), dtype=torch.int64)),
                          ("dbls", torch.empty((n, 4), dtype=torch.float64)),
                          ("rng", torch.empty((n, MSE_SNAP_RNG_WORDS), dtype=torch.int64)),
                          ("seeds", torch.empty((n,), dtype=torch.int64))):
            check_tensor(sd, key, like, "BatchedSortingEnv")
        if isinstance(sd.get("policy_step"), bool) or not isinstance(sd.get("policy_step"), int) or sd["policy_step"] < 0:
            raise ValueError(f"BatchedSortingEnv: policy_step must be a non-negative int, the checkpoint has {sd.get('policy_step')!r}")

    def load_state_dict(self, sd: dict) -> None:
        """`check_state_dict`, then `set_state`, `policy_step`, `seeds` and `refresh_outputs()`: `obs` / `mask` are those
        of the restored state; `reward` / `done` / `terminal_obs` keep whatever the last step here wrote."""
        self.check_state_dict(sd)
        self.set_state(sd["ints"], sd["dbls"], sd["rng"])
        self.policy_step = sd["policy_step"]
        self.seeds.copy_(sd["seeds"])
        self.refresh_outputs()

    def error_count(self) -> int:
        v = C.c_uint64(0)
        check(self.L.mse_error_count(self._h, C.byref(v)))
        return int(v.value)

    @property
    def algorithmic_bytes_per_step(self) -> int:
        return int(self.L.mse_algorithmic_bytes_per_step(self._h))
