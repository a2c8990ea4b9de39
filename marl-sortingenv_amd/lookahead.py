"""A planner on the step engine: the textbook rollout algorithm with the simulator as its model.

From the current state of every env, try every action, follow each with horizon - 1 steps of a base policy, and take the
action with the best return.  `BatchedSortingEnv.lookahead` is that in one launch (`mse_lookahead`: every env's state is
read once, the A x M forks run in registers, nothing is written back).  With an `MlpPolicy` as `base_policy` and / or
`leaf_value` it is `mse_lookahead_net`: the learned actor inside the fork, the learned critic at its end.  On top of it:

- `lookahead_reference`: the multi-launch twin, written from include/mse.h's sentence with calls that exist without the
  kernel - a scratch env of N x A x M forks filled by `get_state` / `set_state`, stepped with `step`, `rule_actions` and
  `sample_actions`; it is what the kernel is tested against, bit for bit;
- `LookaheadCollector`: `DemonstrationCollector` with the planner as the teacher - its dict feeds `ImitationLearner`;
- `evaluate_lookahead`: the planner as an action source under SB3's episode counting rule (`EpisodeStats`).

PyTorch is plumbing (device memory, the stream, copies into buffers; in the twin also the float64 bookkeeping of the returns);
there is no CPU fallback.
"""
from __future__ import annotations

from typing import Optional

import torch

from ._lib import check
from .batched import BatchedSortingEnv, lookahead_network
from .collector import rollout_buffers
from .episodes import _begin, _finish
from .learner import _ptr, _stream
from .policy import MlpPolicy

LOOKAHEAD_KW = ("gamma", "base_policy", "streams", "seed", "base_seed", "n_samples", "sort_mode", "check_overflow", "leaf_value",
                "base_deterministic")
LOOKAHEAD_ROWS = ("observations", "action_masks", "actions", "stepped_actions", "rewards", "episode_starts", "returns")


def check_lookahead_args(horizon: int, kw: dict, allowed=LOOKAHEAD_KW) -> None:
    """ValueError / TypeError for what `BatchedSortingEnv.lookahead` would refuse, before anything is stepped."""
    unknown = sorted(set(kw) - set(allowed))
    if unknown:
        raise TypeError(f"unknown lookahead argument(s) {unknown}: the choices are {list(allowed)}")
    if int(horizon) < 1:
        raise ValueError("horizon must be >= 1")
    lookahead_network(kw.get("base_policy", "rule_based"), kw.get("leaf_value"))  # a bad string, two different policies
    if kw.get("streams", "fresh") not in ("fresh", "own"):
        raise ValueError(f"streams must be 'fresh' or 'own', not {kw['streams']!r}")
    if int(kw.get("n_samples", 1)) < 1:
        raise ValueError("n_samples must be >= 1")


def _scratch_like(env: BatchedSortingEnv, num_envs: int, index_offset: int = 0, seeds=None) -> BatchedSortingEnv:
    """A handle with `env`'s config and auto_reset on; without `seeds` it holds no episode until `set_state`."""
    c = env._cfg_struct
    return BatchedSortingEnv(env.kind, num_envs=num_envs, device=env.device, seeds=seeds, max_steps=env.max_steps,
                             noise_sorting=float(c.noise), balesize=int(c.bale_standard_size), config=env.config, auto_reset=True,
                             track_bales=bool(c.track_bales), literal_choice=bool(c.literal_choice), index_offset=index_offset,
                             reset_now=seeds is not None, rollout_pipeline=2)


def stream_seeds(env: BatchedSortingEnv, seed: int, n_samples: int) -> torch.Tensor:
    """i64[M, N] (host): `mse_lookahead_stream_seed(seed, index_offset + i, m)`."""
    f = env.L.mse_lookahead_stream_seed
    return torch.tensor([[int(f(int(seed), env.index_offset + i, m)) for i in range(env.num_envs)] for m in range(int(n_samples))],
                        dtype=torch.int64)


def lookahead_reference(env: BatchedSortingEnv, horizon: int, gamma: float = 1.0, base_policy="rule_based",
                        streams: str = "fresh", seed: int = 0, base_seed: int = 2024, n_samples: int = 1,
                        sort_mode: Optional[torch.Tensor] = None, check_overflow: bool = False,
                        leaf_value: Optional[MlpPolicy] = None, base_deterministic: bool = True) -> dict:
    """`env.lookahead(...)` in many launches; the same dict.  Fork j = (m * A + a) * N + i is env i under candidate a in
    sample m.  `env` is only read (`get_state`, `action_masks`).  A network base policy is `policy.forward` on the scratch
    env's observation and mask, block by block over the A x M blocks of N forks (a block's rows are envs 0 .. N - 1, so
    `index_offset=env.index_offset` gives fork j the word of env i); the leaf is `forward(...)["value"]` of the state the
    forks stand in after `horizon` steps, added where no step ended the fork's episode."""
    check_lookahead_args(horizon, dict(base_policy=base_policy, streams=streams, n_samples=n_samples, leaf_value=leaf_value))
    net, base_code = lookahead_network(base_policy, leaf_value)
    N, A, M, dev = env.num_envs, env.num_actions, int(n_samples), env.device
    F = N * A * M
    ints, dbls, rng = env.get_state()
    legal = env.action_masks().t().ne(0)  # [A, N]
    rep = lambda t: t.repeat(A * M, 1)  # noqa: E731  the record of env i in every fork of it
    fork_rng = rep(rng)
    if streams == "fresh":  # every stream column is the one reset(seed=...) gives; the rest of the record stays the env's
        helper = _scratch_like(env, N * M, seeds=stream_seeds(env, seed, M).reshape(-1))
        fork_rng = helper.get_state()[2].view(M, 1, N, -1).expand(M, A, N, -1).reshape(F, -1)
        helper.close()
    scratch = _scratch_like(env, F)
    scratch.set_state(rep(ints), rep(dbls), fork_rng)
    sm = None if sort_mode is None else sort_mode.to(device=dev, dtype=torch.int32).repeat(A * M)
    sampler = _scratch_like(env, N, index_offset=env.index_offset) if base_code == 0 and horizon > 1 else None
    fwd = None  # the network's output dict of one block, written again by every forward

    # step 0: the candidate; a forbidden candidate's fork steps the env's first legal action instead and is discarded below
    cand = torch.arange(A, dtype=torch.int32, device=dev).view(A, 1).expand(A, N)
    first_legal = legal.to(torch.int32).argmax(dim=0, keepdim=True).to(torch.int32).expand(A, N)
    actions = torch.where(legal, cand, first_legal).repeat(M, 1).reshape(F).contiguous()
    acc = torch.zeros(F, dtype=torch.float64, device=dev)
    alive = torch.ones(F, dtype=torch.bool, device=dev)
    disc = 1.0
    for s in range(int(horizon)):
        if s > 0:
            if base_code == 1:
                actions = scratch.rule_actions()
            elif base_code == 2:  # mse_policy_forward on the fork's observation and action_masks(), t = s
                actions = torch.empty(F, dtype=torch.int32, device=dev)
                for b in range(A * M):
                    cut = slice(b * N, (b + 1) * N)
                    fwd = net.forward(scratch.obs[cut], scratch.mask[cut], seed=base_seed, t=s, deterministic=bool(base_deterministic),
                                      index_offset=env.index_offset, out=fwd)
                    actions[cut] = fwd["action"]
            else:  # the word of (base_seed, global index of env i, s): the same for every fork of env i
                si, sd, sr = scratch.get_state()
                sampler.policy_step = s
                actions = torch.empty(F, dtype=torch.int32, device=dev)
                for b in range(A * M):
                    cut = slice(b * N, (b + 1) * N)
                    sampler.set_state(si[cut], sd[cut], sr[cut])
                    actions[cut] = sampler.sample_actions(base_seed)
        scratch.step(actions, sort_mode=sm, check_overflow=check_overflow, want_reward64=True)
        acc = torch.where(alive, acc + disc * scratch.reward64, acc)  # acc += disc * r: two roundings
        alive = alive & scratch.done.eq(0)  # the fork ends with its episode; the scratch env's auto-reset is not looked at
        disc = disc * float(gamma)
        if not bool(alive.any()):
            break
    if leaf_value is not None and bool(alive.any()):  # `alive` forks took `horizon` steps; disc = gamma^horizon, rounded per step
        leaf = torch.empty(F, dtype=torch.float64, device=dev)
        for b in range(A * M):
            cut = slice(b * N, (b + 1) * N)
            fwd = net.forward(scratch.obs[cut], scratch.mask[cut], seed=base_seed, t=int(horizon), deterministic=True,
                              index_offset=env.index_offset, out=fwd)
            leaf[cut] = fwd["value"].double()
        acc = torch.where(alive, acc + disc * leaf, acc)  # ret + disc * (double)v: two roundings
    scratch.close()
    if sampler is not None:
        sampler.close()
    ret = acc.view(M, A, N)
    total = ret[0].clone()
    for m in range(1, M):
        total = total + ret[m]
    # a tensor divisor: torch turns division by a Python scalar into a multiplication by its reciprocal, which is not "/ M"
    q = torch.where(legal, total / torch.full_like(total, float(M)), torch.full_like(total, float("-inf")))
    value = q.max(dim=0).values
    index = torch.arange(A, dtype=torch.int32, device=dev).view(A, 1).expand(A, N)
    action = torch.where(q.eq(value.view(1, N)), index, torch.full_like(index, A)).min(dim=0).values  # ties: the lowest
    return {"q": q.contiguous(), "action": action.to(torch.int32).contiguous(), "value": value.contiguous()}


class LookaheadCollector:
    """`DemonstrationCollector` with the planner as the teacher.  Per step k (t = steps collected so far):

        la = env.lookahead(horizon, gamma=gamma, seed=seed + t, **lookahead_kw)     # the env is not touched
        observations[k], action_masks[k], episode_starts[k] = env.obs, env.mask, dones of the step before
        actions[k], values[k] = la["action"], la["value"]                           # the planner's label and its q
        rule_actions[k] = env.rule_actions()                                        # what the rule would do there
        stepped = la["action"]                                       if actor is None
                  actor.forward(env.obs, env.mask, seed=seed, t=t)   otherwise (argmax with deterministic_actor)
        stepped_actions[k] = stepped;  rewards[k], dones = env.step(stepped)        # sort_mode / check_overflow as planned

    then `returns` = `mse_gae` with zero values and lambda = 1 over the window (`DemonstrationCollector`'s).  `collect()`
    returns that collector's dict - `observations`, `action_masks`, `actions`, `rewards`, `episode_starts`, `last_dones`,
    `returns`, `stepped_actions` - plus `rule_actions` i32[K, N] and `values` f64[K, N]; `ImitationLearner.learn` consumes
    it unchanged, and since it steps through `mse_step`, `evaluate_plant`'s trace and `EpisodeStats` see it as any stepping.
    gamma discounts both the planner's returns and `returns`.  lookahead_kw: base_policy, streams, base_seed, n_samples,
    sort_mode, check_overflow, leaf_value, base_deterministic.  base_policy and leaf_value may be an `MlpPolicy`
    (`mse_lookahead_net`): the handle is live, so every `env.lookahead` of the loop above plans with the weights the policy
    holds at that moment.  `LookaheadCollector(env, ..., actor=student, base_policy=student, leaf_value=student)` followed by
    `ImitationLearner(student).learn` is expert iteration: the student steps the env, is the base policy and the leaf value
    of the planner that labels it, and each `collect()` plans with what the last update left."""

    def __init__(self, env: BatchedSortingEnv, n_steps: int, horizon: int, actor: Optional[MlpPolicy] = None,
                 deterministic_actor: bool = False, gamma: float = 0.99, seed: int = 2024, **lookahead_kw):
        check_lookahead_args(horizon, lookahead_kw, allowed=tuple(k for k in LOOKAHEAD_KW if k not in ("gamma", "seed")))
        if int(n_steps) < 1:
            raise ValueError("n_steps must be >= 1")
        if not env.auto_reset:
            raise ValueError("collection needs auto_reset=True (episodes end inside a rollout)")
        if actor is not None and (actor.obs_dim != env.obs_dim or actor.n_actions != env.num_actions):
            raise ValueError(f"the actor must be a {env.obs_dim} -> {env.num_actions} policy")
        self.env, self.actor, self.horizon = env, actor, int(horizon)
        self.deterministic_actor, self.gamma = bool(deterministic_actor), float(gamma)
        self.n_steps, self.seed, self.t = int(n_steps), int(seed), 0
        self.lookahead_kw = dict(lookahead_kw)
        n, K, dev = env.num_envs, self.n_steps, env.device
        self.buffers = rollout_buffers(env, K, names=LOOKAHEAD_ROWS)
        self.buffers["rule_actions"] = torch.empty((K, n), dtype=torch.int32, device=dev)
        self.buffers["values"] = torch.empty((K, n), dtype=torch.float64, device=dev)
        self._zeros = torch.zeros((K + 1, n), dtype=torch.float32, device=dev)  # mse_gae's values and last_values
        self._adv = torch.empty((K, n), dtype=torch.float32, device=dev)
        self._last_done = torch.ones((n,), dtype=torch.uint8, device=dev)  # the envs were just reset
        self._out, self._la = None, None

    def collect(self) -> dict:
        env, b, K, kw = self.env, self.buffers, self.n_steps, self.lookahead_kw
        for k in range(K):
            self._la = la = env.lookahead(self.horizon, gamma=self.gamma, seed=self.seed + self.t, out=self._la, **kw)
            b["observations"][k].copy_(env.obs)
            b["action_masks"][k].copy_(env.mask)
            b["episode_starts"][k].copy_(self._last_done)
            b["actions"][k].copy_(la["action"])
            b["values"][k].copy_(la["value"])
            b["rule_actions"][k].copy_(env.rule_actions())
            if self.actor is None:
                stepped = la["action"]
            else:
                self._out = self.actor.forward(env.obs, env.mask, seed=self.seed, t=self.t, deterministic=self.deterministic_actor,
                                               index_offset=env.index_offset, out=self._out)
                stepped = self._out["action"]
            b["stepped_actions"][k].copy_(stepped)
            _, rew, done, _ = env.step(b["stepped_actions"][k], sort_mode=kw.get("sort_mode"),
                                       check_overflow=bool(kw.get("check_overflow", False)))
            b["rewards"][k].copy_(rew)
            self._last_done.copy_(done)
            self.t += 1
        last_dones = self._last_done.clone()
        with torch.cuda.device(env.device):
            check(env.L.mse_gae(K, env.num_envs, _ptr(b["rewards"]), _ptr(self._zeros), _ptr(b["episode_starts"]),
                                _ptr(self._zeros[K]), _ptr(last_dones), self.gamma, 1.0, _ptr(self._adv), _ptr(b["returns"]),
                                _stream(env.device)))
        return dict(b, last_dones=last_dones)


def evaluate_lookahead(env: BatchedSortingEnv, n_eval_episodes: int, horizon: int, **lookahead_kw):
    """`evaluate_rollout` with the planner as the action source: the env is reset with its own `seeds` and its policy step
    counter set to 0; at step t every env takes `env.lookahead(horizon, seed=seed + t, ...)["action"]` (seed: lookahead_kw's,
    default 0); env i contributes its first (n_eval_episodes + i) // N episodes (`EpisodeStats` with SB3's targets, one scan
    per max_steps steps).  Returns (mean, std) of the episode returns."""
    kw = dict(lookahead_kw)
    check_lookahead_args(horizon, kw)
    seed = int(kw.pop("seed", 0))
    stats, most = _begin(env, n_eval_episodes, None)
    K = env.max_steps
    buf = {"reward": torch.empty((K, env.num_envs), dtype=torch.float32, device=env.device),
           "done": torch.empty((K, env.num_envs), dtype=torch.uint8, device=env.device)}
    la, t = None, 0
    for _ in range(most):
        for k in range(K):
            la = env.lookahead(horizon, seed=seed + t, out=la, **kw)
            _, rew, done, _ = env.step(la["action"], sort_mode=kw.get("sort_mode"), check_overflow=bool(kw.get("check_overflow", False)))
            buf["reward"][k].copy_(rew)
            buf["done"][k].copy_(done)
            t += 1
        stats.update(buf)
    return _finish(stats, n_eval_episodes, False)
