"""The learner's half of PPO on the device (SB3's `model.learn` -> `MaskablePPO.train`, src/training.py:191).

`compute_gae` is `RolloutBuffer.compute_returns_and_advantage` on a collector's buffers (`mse_gae`), and
`PPOLearner.update` is `MaskablePPO.train` on them: per minibatch one `mse_ppo_loss_grad` (loss, its statistics and
the gradient w.r.t. all weights, three launches) and one `mse_ppo_adam_step` (clip_grad_norm_ + Adam), all enqueued
without a host synchronisation; the new weights go back into the policy the rollout kernels read once per update
(`MlpPolicy.load_weights`, or with `weight_sync="device"` one repack launch, `MlpPolicy.load_weights_device`).  SB3's
`target_kl` early stop is a flag on the device that the gated entry points read (`mse_ppo_loss_grad_gated`).  PyTorch is plumbing (device memory, the stream, the seeded permutation); no torch op
computes anything on this path, and there is no CPU fallback.  With `shuffle="device"` the permutation is a kernel too
(`mse_ppo_shuffle`, a counter-based function of seed and epoch that `PPOLearner.permutation` replays on the host).
SB3's `clip_range_vf` is a second instantiation of either gradient kernel (`mse_ppo_loss_grad_vclip`), its schedules are
host arithmetic on `progress_remaining` (`resolve_schedule`), and `train/explained_variance` is one more small kernel per
update (`mse_explained_variance`).
`bc_coef` adds an imitation term to the loss (`mse_ppo_bc_loss_grad`: the rule-based controller's labels of the rollout's own
states, `data["expert_actions"]`, in the same gradient launch), so that fine-tuning a cloned policy does not forget its teacher.
`learn` can report the reference's unit, cumulative reward per episode (episodes.py): SB3's `rollout/ep_rew_mean` from an
`EpisodeStats` over the training rollouts, and `EvalCallback`'s periodic `evaluate_policy` with the best weights kept.
`state_dict` / `load_state_dict` carry everything of a run that lives here, and `learn(first_iteration=...,
checkpoint_path=..., checkpoint_freq=...)` writes and continues whole runs (checkpoint.py): a resumed run is the same run.
`exchange` (a `sharding.GradientExchange`) makes the update data-parallel: every rank keeps the rollout rows it collected and
a minibatch is cut into three phases (`mse_ppo_shard_moments`, `mse_ppo_shard_loss_grad`, `mse_ppo_shard_finish`) with one
all-reduce of four doubles and one of the gradient sums between them; no rollout row crosses a link.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Callable, Optional, Union

import torch

from ._lib import MsePpoParams, check, load_library
from .checkpoint import format_path, save_checkpoint
from .episodes import EpisodeStats, evaluate_policy
from .policy import MlpPolicy

STAT_NAMES = ("loss", "policy_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction", "adv_mean", "adv_std")
# the columns with `bc_coef` set (`mse_ppo_bc_loss_grad`): `loss` then includes bc_coef * bc_loss; the last one is always 0
PPO_BC_STAT_NAMES = STAT_NAMES + ("bc_loss", "bc_accuracy", "bc_unusable", "reserved")


def _ptr(x):
    return None if x is None else C.c_void_p(x.data_ptr())


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


Schedule = Union[float, Callable[[float], float]]


def resolve_schedule(value: Schedule, progress_remaining: float, name: str = "value", allow_zero: bool = False) -> float:
    """SB3's schedule convention, with no device in it: `value` is a number, or a function of `progress_remaining` (1 at
    the start of training, 0 at its end) that is called with it.  -> the value as a Python float.  A result that is not
    finite or not positive is refused (ValueError naming `name`); allow_zero=True admits 0, which a linear decay of
    `learning_rate` or `clip_range` reaches in its last update (`clip_range_vf` must stay above 0: 0 would mean "off")."""
    v = float(value(float(progress_remaining)) if callable(value) else value)
    if not math.isfinite(v) or v < 0.0 or (v == 0.0 and not allow_zero):
        raise ValueError(f"{name} must be finite and {'>= 0' if allow_zero else '> 0'}, not {v!r} "
                         f"(progress_remaining = {float(progress_remaining)!r})")
    return v


def compute_gae(data: dict, gamma: float = 0.99, gae_lambda: float = 0.95) -> dict:
    """Adds `advantages` and `returns` f32[K, N] to a collector's dict (`rewards`, `values`, `episode_starts` [K, N],
    `last_values`, `last_dones` [N], device tensors): SB3's compute_returns_and_advantage, bit for bit."""
    r = data["rewards"]
    if not r.is_cuda:
        raise RuntimeError("compute_gae needs device tensors: there is no CPU fallback")
    K, n = r.shape
    L = load_library()
    names = ("rewards", "values", "episode_starts", "last_values", "last_dones")
    dtypes = (torch.float32, torch.float32, torch.uint8, torch.float32, torch.uint8)
    t = [data[k].to(device=r.device, dtype=d).contiguous() for k, d in zip(names, dtypes)]
    if tuple(t[1].shape) != (K, n) or tuple(t[2].shape) != (K, n) or tuple(t[3].shape) != (n,) or tuple(t[4].shape) != (n,):
        raise ValueError("rollout buffers must be [K, N] with last_values / last_dones [N]")
    adv = data.get("advantages")
    ret = data.get("returns")
    if adv is None or adv.shape != r.shape or adv.dtype != torch.float32 or not adv.is_contiguous():
        adv = torch.empty_like(t[0])
    if ret is None or ret.shape != r.shape or ret.dtype != torch.float32 or not ret.is_contiguous():
        ret = torch.empty_like(t[0])
    with torch.cuda.device(r.device):
        check(L.mse_gae(K, n, _ptr(t[0]), _ptr(t[1]), _ptr(t[2]), _ptr(t[3]), _ptr(t[4]), float(gamma), float(gae_lambda),
                        _ptr(adv), _ptr(ret), _stream(r.device)))
    data["advantages"], data["returns"] = adv, ret
    return data


def training_loop(iterations: int, collect, step, first_iteration: Optional[int] = None, history: Optional[list] = None,
                  stats_owner=None, stats_device=None, evaluate=None, eval_freq: int = 0, checkpoint=None,
                  checkpoint_freq: int = 0, callback=None) -> list:
    """The loop of `PPOLearner.learn`, `ImitationLearner.learn` and `ModularTrainer.learn`, defined once: for `it` in
    range(first_iteration, iterations) (None: from 0, unchecked) `data = collect(it)` and `rec = step(data, 1 - (it + 1) /
    iterations)`.  With `stats_owner` its `episode_stats` (created on `stats_device` when absent or of another width) books
    the rollout before `step`, and rec gains `episodes`, `ep_rew_mean`, `ep_len_mean` after it; every eval_freq-th rec
    gains `eval_mean_reward`, `eval_std_reward` = `evaluate()`.  Then, always in this order: `history.append(rec)`,
    every checkpoint_freq-th iteration `checkpoint(it + 1, history)`, `callback(it, rec)`.  -> history (a copy, extended)."""
    iterations, eval_freq, checkpoint_freq = int(iterations), int(eval_freq), int(checkpoint_freq)
    if first_iteration is not None and not 0 <= int(first_iteration) <= iterations:
        raise ValueError(f"first_iteration must be in [0, iterations = {iterations}], not {first_iteration!r}")
    if checkpoint_freq < 0 or (checkpoint_freq > 0 and checkpoint is None):
        raise ValueError("checkpoint_freq must be >= 0, and > 0 needs a checkpoint_path")
    history = [] if history is None else list(history)
    for it in range(int(first_iteration or 0), iterations):
        data = collect(it)
        if stats_owner is not None:
            n = data["rewards"].shape[1]
            if stats_owner.episode_stats is None or stats_owner.episode_stats.num_envs != n:
                stats_owner.episode_stats = EpisodeStats(n, stats_device)
            stats_owner.episode_stats.reset_totals()
            stats_owner.episode_stats.update(data)
        rec = step(data, 1.0 - (it + 1) / iterations)
        if stats_owner is not None:
            t = stats_owner.episode_stats.totals()
            rec.update(episodes=t["episodes"], ep_rew_mean=t["mean_return"], ep_len_mean=t["mean_length"])
        if evaluate is not None and eval_freq > 0 and (it + 1) % eval_freq == 0:
            mean, std = evaluate()
            rec.update(eval_mean_reward=mean, eval_std_reward=std)
        history.append(rec)
        if checkpoint_freq > 0 and (it + 1) % checkpoint_freq == 0:
            checkpoint(it + 1, history)
        if callback is not None:
            callback(it, rec)
    return history


class PPOLearner:
    """SB3's PPO defaults (the reference overrides ent_coef=0.05, src/training.py:115-131).  `batch_size=None`: 64 rows
    per env-step-column is far too small for a 10^6-row rollout, so the default is K * N / 4 rounded up - pass SB3's 64
    explicitly to reproduce its schedule.

    `shuffle="cpu"` (the default) permutes the rows of each epoch with `torch.randperm` on a seeded CPU generator and
    copies the indices up; `last_permutations` keeps them.  `shuffle="device"` fills one i64[K * N] device buffer per
    epoch with `mse_ppo_shuffle(total, seed, epochs_done, ...)` on the current stream: no host work, no copy.
    `epochs_done` counts the epochs of the learner's lifetime, so no two share a permutation; `last_epochs` lists the
    counters the last `update()` used and `permutation(total, epoch)` returns the same rows on the CPU.

    `weight_sync="host"` (the default) hands the new weights to the policy through the host (`load_weights`: a copy down,
    the host repack, a blocking copy up); `"device"` enqueues `load_weights_device` behind the last Adam step, so an
    update ends in the one small copy of its statistics and `policy.sync()`.  Same weights, same image, bit for bit.

    `target_kl` (SB3's; None = off): after a minibatch whose approx_kl exceeds 1.5 * target_kl that minibatch takes no
    optimiser step and no later minibatch of the update runs.  The decision is taken on the device: `update()` still
    enqueues every minibatch, the ones after the stop exit at once, and the result says what ran.  `step` counts the
    Adam steps actually taken; `epochs_done` advances by the epochs ENQUEUED (n_epochs per update), run or not.

    `arithmetic="fma"` (the default) forms the gradient's products as fmaf chains on the vector unit
    (`mse_ppo_loss_grad`); `"matrix"` forms them on the f32 matrix cores (`mse_ppo_loss_grad_matrix`): the same per-row
    arithmetic, sums in another order, so the two agree within rounding and each is reproducible bit for bit.

    `clip_range_vf` (SB3's; None = off): the value loss is that of `old + clamp(value - old, -c, c)` with `old` the
    rollout's `data["values"]`; every `loss_grad` then goes through `mse_ppo_loss_grad_vclip`, with either arithmetic,
    gated or not.  With None `loss_grad` calls exactly what it called without the argument.

    `learning_rate`, `clip_range` and `clip_range_vf` may each be a function of `progress_remaining` (SB3's schedules;
    `resolve_schedule`).  `progress_remaining` (1.0 until set) is the progress used: `update(data, progress_remaining=p)`
    sets it, `learn` sets it to `1 - (it + 1) / iterations` before update `it` - SB3's order, in which `num_timesteps`
    has already counted the rollout about to be trained on, so the last update of a linear schedule runs at 0.  The three
    are evaluated once at the top of each `update()` into `learning_rate` (the `lr` of the Adam launches), `clip_range`
    (written into `params`) and `clip_range_vf`.  With plain numbers nothing is evaluated and nothing changes.

    `bc_coef` (None = off; a number >= 0 or a schedule, which may reach 0): the minibatch loss gains `bc_coef * bc_loss`,
    the cross-entropy of the rule-based controller's action under the policy's masked softmax at every rollout row (DAPG /
    kickstarting).  Every `loss_grad` then goes through `mse_ppo_bc_loss_grad`, with either arithmetic, gated or not, with
    or without `clip_range_vf`, and reads `data["expert_actions"]` (i32, one per row: the collectors' `expert_labels=True`).
    A row whose label the mask forbids adds nothing to that term.  The statistics have twelve columns (PPO_BC_STAT_NAMES).
    With None everything is exactly what it was without the argument.

    `exchange` (None = off; a `sharding.GradientExchange`): a data-parallel update over the ranks of its group.  Every rank
    constructs the learner over its own policy and passes `update()` the rollout of its own envs (`ShardedSortingEnv.env`
    under a `FusedPolicyRollout`); GAE stays local, because it is per env.  The constructor broadcasts rank 0's weights, so
    all ranks start alike (`m` and `v` are zero everywhere), and the shuffle seed becomes `(seed + rank) mod 2^64`, so ranks
    do not permute alike (`permutation()` and the CPU generator use that seed).  `batch_size` counts rows PER RANK; the
    minibatches of an epoch are `shard_minibatch_plan(totals, batch_size)` over the ranks' row counts, so with ragged shards
    a rank meets short and empty minibatches and still makes every collective call.  Per minibatch: `shard_moments` ->
    `all_reduce_sum` -> `shard_partial` -> `all_reduce_sum` -> `shard_finish` -> the Adam step; every rank finishes from the
    same summed bits, so weights, `m`, `v`, the `target_kl` decision and the returned statistics (the GLOBAL minibatch's) are
    identical on all ranks without ever being exchanged.  A checkpoint is per rank.
    RESULTS ARE NOT INDEPENDENT OF THE NUMBER OF RANKS (unlike the env engine's rollouts, which are): which rows share a
    minibatch is decided per rank, and the sums are formed in another order.  A given world size is reproducible bit for bit.
    `bc_coef` and `update(explained_variance=True)` are refused together with an exchange.
    With None the learner is exactly what it was without the argument."""

    bc_coef: Optional[float] = None  # off unless the constructor sets it
    exchange = None  # off unless the constructor sets it

    def __init__(self, policy: MlpPolicy, learning_rate: Schedule = 3e-4, n_epochs: int = 10, batch_size: Optional[int] = None,
                 gamma: float = 0.99, gae_lambda: float = 0.95, clip_range: Schedule = 0.2, ent_coef: float = 0.0,
                 vf_coef: float = 0.5, max_grad_norm: float = 0.5, normalize_advantage: bool = True, adam_eps: float = 1e-5,
                 seed: int = 0, shuffle: str = "cpu", weight_sync: str = "host", target_kl: Optional[float] = None,
                 arithmetic: str = "fma", clip_range_vf: Optional[Schedule] = None, bc_coef: Optional[Schedule] = None,
                 exchange=None):
        if exchange is not None and bc_coef is not None:
            raise ValueError("bc_coef cannot be combined with an exchange: mse_ppo_bc_loss_grad has no sharded form")
        if shuffle not in ("cpu", "device"):
            raise ValueError(f"shuffle must be 'cpu' or 'device', not {shuffle!r}")
        if weight_sync not in ("host", "device"):
            raise ValueError(f"weight_sync must be 'host' or 'device', not {weight_sync!r}")
        if arithmetic not in ("fma", "matrix"):
            raise ValueError(f"arithmetic must be 'fma' or 'matrix', not {arithmetic!r}")
        self.weight_sync = weight_sync
        self.arithmetic = arithmetic
        self.target_kl = None if target_kl is None else float(target_kl)
        # a callable is kept as the schedule and evaluated at progress 1 for now; update() re-evaluates it
        self.progress_remaining = 1.0
        self.schedules = {name: v for name, v in (("learning_rate", learning_rate), ("clip_range", clip_range),
                                                  ("clip_range_vf", clip_range_vf), ("bc_coef", bc_coef)) if callable(v)}
        if "learning_rate" in self.schedules:
            learning_rate = resolve_schedule(learning_rate, 1.0, "learning_rate", allow_zero=True)
        if "clip_range" in self.schedules:
            clip_range = resolve_schedule(clip_range, 1.0, "clip_range", allow_zero=True)
        self.clip_range = float(clip_range)
        self.clip_range_vf = None if clip_range_vf is None else resolve_schedule(clip_range_vf, 1.0, "clip_range_vf")
        self.bc_coef = None if bc_coef is None else resolve_schedule(bc_coef, 1.0, "bc_coef", allow_zero=True)
        self.policy, self.L = policy, policy.L
        self.learning_rate, self.n_epochs, self.batch_size = float(learning_rate), int(n_epochs), batch_size
        self.gamma, self.gae_lambda = float(gamma), float(gae_lambda)
        self.max_grad_norm, self.adam_eps = float(max_grad_norm), float(adam_eps)
        self.beta1, self.beta2 = 0.9, 0.999
        self.params = MsePpoParams(C.sizeof(MsePpoParams), float(clip_range), float(ent_coef), float(vf_coef),
                                   1 if normalize_advantage else 0)
        self.exchange = exchange
        if exchange is not None:  # ranks must not permute alike
            seed = (int(seed) + int(exchange.rank)) & (2 ** 64 - 1)
        self.shuffle, self.seed = shuffle, int(seed) & (2 ** 64 - 1)
        self.generator = torch.Generator(device="cpu").manual_seed(int(seed))
        dev = policy.device
        self.device = dev
        self.n_weights = int(self.L.mse_policy_num_weights(policy.obs_dim, policy.n_actions))
        self.weights = torch.from_numpy(policy.flat_weights()).to(dev)  # the flat f32 master copy the kernels train
        self.grad = torch.zeros(self.n_weights, dtype=torch.float32, device=dev)
        self.m = torch.zeros_like(self.grad)
        self.v = torch.zeros_like(self.grad)
        self.grad_norm = torch.zeros(1, dtype=torch.float32, device=dev)
        ws = int((self.L.mse_ppo_workspace_bytes if self.bc_coef is None else self.L.mse_ppo_bc_workspace_bytes)(
            policy.obs_dim, policy.n_actions))
        self.workspace = torch.empty(ws, dtype=torch.uint8, device=dev)
        self.step = 0  # Adam steps taken
        self.last_permutations: list = []  # the CPU permutations of the last update(), one per epoch (shuffle="cpu")
        self.epochs_done = 0  # shuffle="device": epochs shuffled so far, the counter the next permutation is keyed by
        self.last_epochs: list = []  # shuffle="device": the counters of the last update(), one per epoch
        self._perm = None  # shuffle="device": i64[K * N], kept until the rollout size changes
        self.episode_stats = None  # learn(episode_stats=True): the EpisodeStats whose carry spans the iterations
        self.best_mean_reward = float("-inf")  # learn(eval_collector=...): EvalCallback's best model so far
        self.best_weights = None  # f32[W] on the device, a copy of `weights` at the best evaluation
        self._shard_buffers = None  # (moments f64[4], partial f64[partial_len]) of the phase methods, made on first use
        self._shard_totals = None  # exchange: (this rank's row count, every rank's), gathered once per rollout size
        if exchange is not None:
            exchange.broadcast(self.weights)  # all ranks start from rank 0's weights
            self._hand_over()
            self.policy.sync()

    def loss_grad(self, data: dict, rows: Optional[torch.Tensor], batch: int, stats_out: torch.Tensor,
                  weights: Optional[torch.Tensor] = None, grad_out: Optional[torch.Tensor] = None,
                  control: Optional[torch.Tensor] = None, target_kl: float = 0.0) -> torch.Tensor:
        """One `mse_ppo_loss_grad` on the flattened rollout in `data` (which holds advantages / returns); returns the
        gradient tensor.  rows: i64 device tensor of row indices, or None for rows 0 .. batch - 1.
        control: i32[2] device tensor {stopped, minibatches_run}: `mse_ppo_loss_grad_gated` with `target_kl` instead.
        With `arithmetic="matrix"` both go to `mse_ppo_loss_grad_matrix`.  With `clip_range_vf` set, all of them go to
        `mse_ppo_loss_grad_vclip` with `data["values"]` (f32[K, N], contiguous) as the old values.  With `bc_coef` set, all
        of them go to `mse_ppo_bc_loss_grad` with `data["expert_actions"]` (i32[K, N], contiguous) as the labels, and
        stats_out is f32[12]."""
        p = self.policy
        obs = data["observations"]
        n_rows = obs.shape[0] * obs.shape[1] if obs.dim() == 3 else obs.shape[0]
        mask = data.get("action_masks")
        w = self.weights if weights is None else weights
        g = self.grad if grad_out is None else grad_out
        for name in ("observations", "actions", "log_probs", "advantages", "returns"):
            if not data[name].is_contiguous():
                raise ValueError(f"{name} must be contiguous")
        args = (p.obs_dim, p.n_actions, _ptr(w), n_rows, _ptr(rows), int(batch), _ptr(obs), _ptr(mask), _ptr(data["actions"]),
                _ptr(data["log_probs"]), _ptr(data["advantages"]), _ptr(data["returns"]), C.byref(self.params), _ptr(g),
                _ptr(stats_out), _ptr(self.workspace), _stream(self.device))
        old = None
        if self.clip_range_vf is not None:
            old = data["values"]
            if old.dtype != torch.float32 or not old.is_contiguous() or old.numel() != n_rows or old.device != obs.device:
                raise ValueError("clip_range_vf needs data['values']: contiguous f32, one per rollout row, on the rollout's device")
        if self.bc_coef is not None:
            expert = data.get("expert_actions")
            if not isinstance(expert, torch.Tensor) or expert.dtype != torch.int32 or not expert.is_contiguous() \
                    or expert.numel() != n_rows or expert.device != obs.device:
                raise ValueError("bc_coef needs data['expert_actions']: contiguous i32, one per rollout row, on the rollout's "
                                 "device (collect with expert_labels=True: PolicyRolloutCollector or FusedPolicyRollout)")
            with torch.cuda.device(self.device):
                check(self.L.mse_ppo_bc_loss_grad(*args, float(target_kl), _ptr(control), 1 if self.arithmetic == "matrix" else 0,
                                                  _ptr(old), float(self.clip_range_vf or 0.0), _ptr(expert), float(self.bc_coef)))
            return g
        with torch.cuda.device(self.device):
            if old is not None:
                check(self.L.mse_ppo_loss_grad_vclip(*args, float(target_kl), _ptr(control), 1 if self.arithmetic == "matrix" else 0,
                                                     _ptr(old), float(self.clip_range_vf)))
            elif self.arithmetic == "matrix":
                check(self.L.mse_ppo_loss_grad_matrix(*args, float(target_kl), _ptr(control)))
            elif control is None:
                check(self.L.mse_ppo_loss_grad(*args))
            else:
                check(self.L.mse_ppo_loss_grad_gated(*args, float(target_kl), _ptr(control)))
        return g

    # ---- a minibatch in three phases (include/mse.h: mse_ppo_shard_*) ---------------------------------------------------
    def _shard_args(self, data: dict):
        if self.bc_coef is not None:
            raise ValueError("bc_coef has no sharded form: the phase methods serve the PPO loss only")
        obs = data["observations"]
        n_rows = obs.shape[0] * obs.shape[1] if obs.dim() == 3 else obs.shape[0]
        if self._shard_buffers is None:
            n = int(self.L.mse_ppo_shard_partial_len(self.policy.obs_dim, self.policy.n_actions))
            self._shard_buffers = (torch.zeros(4, dtype=torch.float64, device=self.device),
                                   torch.zeros(n, dtype=torch.float64, device=self.device))
        return obs, n_rows

    def shard_moments(self, data: dict, rows: Optional[torch.Tensor], batch_local: int, control: Optional[torch.Tensor] = None,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Phase 1, `mse_ppo_shard_moments`: {batch_local, sum a, sum a^2, 0} over this shard's minibatch rows of
        `data["advantages"]` -> f64[4] on the device (`out`, or a buffer the learner keeps).  rows: i64 device tensor, or
        None for rows 0 .. batch_local - 1; batch_local may be 0.  The caller sums the shards' results."""
        _, n_rows = self._shard_args(data)
        m = self._shard_buffers[0] if out is None else out
        if not data["advantages"].is_contiguous():
            raise ValueError("advantages must be contiguous")
        with torch.cuda.device(self.device):
            check(self.L.mse_ppo_shard_moments(n_rows, _ptr(rows), int(batch_local), _ptr(data["advantages"]), _ptr(m),
                                               _ptr(self.workspace), _stream(self.device), _ptr(control)))
        return m

    def shard_partial(self, data: dict, rows: Optional[torch.Tensor], batch_local: int, global_batch: int, moments: torch.Tensor,
                      control: Optional[torch.Tensor] = None, target_kl: float = 0.0, weights: Optional[torch.Tensor] = None,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Phase 2, `mse_ppo_shard_loss_grad`: this shard's gradient and statistic sums of a minibatch of `global_batch`
        rows over all shards, with the advantages normalised by `moments` (f64[4], device: the SUM of all shards' phase 1)
        -> f64[partial_len] on the device (`out`, or a buffer the learner keeps).  `arithmetic` and `clip_range_vf` (with
        `data["values"]`) apply as in `loss_grad`.  target_kl is not read here (the gate's decision is phase 3's).  The
        caller sums the shards' results."""
        p = self.policy
        obs, n_rows = self._shard_args(data)
        out = self._shard_buffers[1] if out is None else out
        w = self.weights if weights is None else weights
        for name in ("observations", "actions", "log_probs", "advantages", "returns"):
            if not data[name].is_contiguous():
                raise ValueError(f"{name} must be contiguous")
        old = None
        if self.clip_range_vf is not None:
            old = data["values"]
            if old.dtype != torch.float32 or not old.is_contiguous() or old.numel() != n_rows or old.device != obs.device:
                raise ValueError("clip_range_vf needs data['values']: contiguous f32, one per rollout row, on the rollout's device")
        with torch.cuda.device(self.device):
            check(self.L.mse_ppo_shard_loss_grad(
                p.obs_dim, p.n_actions, _ptr(w), n_rows, _ptr(rows), int(batch_local), _ptr(obs), _ptr(data.get("action_masks")),
                _ptr(data["actions"]), _ptr(data["log_probs"]), _ptr(data["advantages"]), _ptr(data["returns"]),
                C.byref(self.params), int(global_batch), _ptr(moments), _ptr(out), _ptr(self.workspace), _stream(self.device),
                _ptr(control), 1 if self.arithmetic == "matrix" else 0, _ptr(old), float(self.clip_range_vf or 0.0)))
        return out

    def shard_finish(self, global_batch: int, reduced: torch.Tensor, moments: torch.Tensor, stats_out: torch.Tensor,
                     control: Optional[torch.Tensor] = None, target_kl: float = 0.0,
                     grad_out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Phase 3, `mse_ppo_shard_finish`: the summed partial and moments -> the gradient (f32[W]: `grad_out`, or
        `self.grad`) and stats_out f32[8]; with `control` it counts the minibatch and takes the `target_kl` decision.
        Returns the gradient tensor; `adam_step` follows."""
        if self.bc_coef is not None:
            raise ValueError("bc_coef has no sharded form: the phase methods serve the PPO loss only")
        g = self.grad if grad_out is None else grad_out
        with torch.cuda.device(self.device):
            check(self.L.mse_ppo_shard_finish(self.policy.obs_dim, self.policy.n_actions, int(global_batch), _ptr(reduced),
                                              _ptr(moments), C.byref(self.params), _ptr(g), _ptr(stats_out), _stream(self.device),
                                              float(target_kl), _ptr(control)))
        return g

    def adam_step(self, control: Optional[torch.Tensor] = None):
        """One Adam step; with `control`, `mse_ppo_adam_step_gated`: nothing happens on the device once it says stopped
        (`step` still advances here: `update()` corrects it from the control block)."""
        self.step += 1
        args = (self.n_weights, _ptr(self.weights), _ptr(self.grad), _ptr(self.m), _ptr(self.v), self.step, self.learning_rate,
                self.beta1, self.beta2, self.adam_eps, self.max_grad_norm, _ptr(self.grad_norm), _stream(self.device))
        with torch.cuda.device(self.device):
            if control is None:
                check(self.L.mse_ppo_adam_step(*args))
            else:
                check(self.L.mse_ppo_adam_step_gated(*args, _ptr(control)))

    def _hand_over(self) -> None:
        """The master weights into the policy the rollout kernels read."""
        if self.weight_sync == "device":
            self.policy.load_weights_device(self.weights, sync=False)  # one launch behind the last Adam step
        else:
            self.policy.load_weights(self.weights)  # the device-to-host copy waits for the stream

    def permutation(self, total: int, epoch: int) -> torch.Tensor:
        """The rows of epoch counter `epoch` over a rollout of `total` rows as shuffle="device" orders them: an i64 CPU
        tensor from `mse_ppo_shuffle_host` (the kernel's arithmetic on the host; no device is touched)."""
        rows = torch.empty(int(total), dtype=torch.int64)
        check(self.L.mse_ppo_shuffle_host(int(total), self.seed, int(epoch), 0, int(total), _ptr(rows)))
        return rows

    def _device_permutation(self, total: int) -> torch.Tensor:
        if self._perm is None or self._perm.numel() != total:
            self._perm = torch.empty(total, dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            check(self.L.mse_ppo_shuffle(total, self.seed, self.epochs_done, 0, total, _ptr(self._perm), _stream(self.device)))
        self.last_epochs.append(self.epochs_done)
        self.epochs_done += 1
        return self._perm

    def _minibatches(self, total: int, bs: int):
        """Yields the device row indices of every minibatch of an update, in order: n_epochs permutations of `total` rows
        (`shuffle`; `last_permutations` / `last_epochs` record them), each cut into runs of `bs`, the last maybe short."""
        for perm in self._epoch_permutations(total):
            for start in range(0, total, bs):
                yield perm[start:start + bs]

    def _epoch_permutations(self, total: int):
        """Yields the device permutation of `total` rows of each of the n_epochs epochs of an update."""
        self.last_permutations, self.last_epochs = [], []
        for _ in range(self.n_epochs):
            if self.shuffle == "device":
                perm = self._device_permutation(total)
            else:
                perm_cpu = torch.randperm(total, generator=self.generator)
                self.last_permutations.append(perm_cpu)
                perm = perm_cpu.to(self.device)
            yield perm

    def _shard_plan(self, total: int):
        """-> (batch size per rank, `shard_minibatch_plan` of one epoch) for a rollout of `total` rows on this rank: one
        all-gather of the ranks' row counts as host integers, repeated only when this rank's rollout size changes."""
        from .sharding import shard_minibatch_plan

        if self._shard_totals is None or self._shard_totals[0] != total:
            self._shard_totals = (total, self.exchange.all_gather_ints(total))
        totals = self._shard_totals[1]
        bs = self.batch_size if self.batch_size is not None else (max(totals) + 3) // 4
        bs = max(1, min(int(bs), max(totals)))
        return bs, shard_minibatch_plan(totals, bs)

    def _sharded_minibatches(self, data: dict, total: int, bs: int, plan: list, stats: torch.Tensor, control) -> None:
        """The minibatch loop of `update()` with an exchange: the three phases with the two all-reduces between them."""
        ex, i = self.exchange, 0
        for perm in self._epoch_permutations(total):
            for j, sizes in enumerate(plan):
                b_local, b_global = sizes[ex.rank], sum(sizes)
                rows = perm[j * bs:j * bs + b_local] if b_local > 0 else None
                # A closed gate still makes both collective calls on every rank (a rank that skipped one would hang the
                # others): the kernels then write nothing, so the buffers that are summed are simply stale, and phase 3,
                # which is closed too, never reads them.
                moments = ex.all_reduce_sum(self.shard_moments(data, rows, b_local, control=control))
                partial = ex.all_reduce_sum(self.shard_partial(data, rows, b_local, b_global, moments, control=control))
                self.shard_finish(b_global, partial, moments, stats[i], control=control, target_kl=self.target_kl or 0.0)
                self.adam_step(control)
                i += 1

    def _resolve_schedules(self) -> None:
        """What SB3 does at the top of train(): the scheduled values at `progress_remaining`, once per update."""
        p = self.progress_remaining
        if "learning_rate" in self.schedules:
            self.learning_rate = resolve_schedule(self.schedules["learning_rate"], p, "learning_rate", allow_zero=True)
        if "clip_range" in self.schedules:
            self.clip_range = resolve_schedule(self.schedules["clip_range"], p, "clip_range", allow_zero=True)
            self.params.clip_range = self.clip_range
        if "clip_range_vf" in self.schedules:
            self.clip_range_vf = resolve_schedule(self.schedules["clip_range_vf"], p, "clip_range_vf")
        if "bc_coef" in self.schedules:
            self.bc_coef = resolve_schedule(self.schedules["bc_coef"], p, "bc_coef", allow_zero=True)

    def explained_variance(self, data: dict, out: torch.Tensor) -> None:
        """One `mse_explained_variance` over all rows of `data["values"]` / `data["returns"]` into `out` (f32[1], device),
        on the current stream, with the learner's workspace (free between two gradient calls, and large enough)."""
        dev = data["returns"].device
        values = data["values"].to(device=dev, dtype=torch.float32).contiguous()
        returns = data["returns"]
        if values.numel() != returns.numel() or returns.dtype != torch.float32 or not returns.is_contiguous():
            raise ValueError("values and returns must be f32 of one size, returns contiguous")
        with torch.cuda.device(self.device):
            check(self.L.mse_explained_variance(returns.numel(), _ptr(values), _ptr(returns), _ptr(out), _ptr(self.workspace),
                                                _stream(self.device)))

    # ---- checkpoint (checkpoint.py) ----------------------------------------------------------------------------------
    def hyperparameters(self) -> dict:
        """Everything the constructor fixes that changes results, as plain data: the dims, the constructor's numbers and
        modes, `scheduled` (the names of the fields that are schedules) and the plain values of the other ones of
        `learning_rate`, `clip_range`, `clip_range_vf`.  `ent_coef` / `vf_coef` are read back from `params`, i.e. as the
        f32 the kernels get.  `bc_coef` is there (as a value, or under `scheduled`) only when it is set, `exchange_world` and
        `exchange_rank` only with an exchange (a checkpoint is per rank)."""
        hp = {"obs_dim": self.policy.obs_dim, "n_actions": self.policy.n_actions, "n_epochs": self.n_epochs,
              "batch_size": None if self.batch_size is None else int(self.batch_size), "gamma": self.gamma,
              "gae_lambda": self.gae_lambda, "ent_coef": float(self.params.ent_coef), "vf_coef": float(self.params.vf_coef),
              "max_grad_norm": self.max_grad_norm, "normalize_advantage": bool(self.params.normalize_advantage),
              "adam_eps": self.adam_eps, "beta1": self.beta1, "beta2": self.beta2, "seed": self.seed, "shuffle": self.shuffle,
              "weight_sync": self.weight_sync, "target_kl": self.target_kl, "arithmetic": self.arithmetic,
              "scheduled": sorted(self.schedules)}
        for name in ("learning_rate", "clip_range", "clip_range_vf"):
            if name not in self.schedules:
                hp[name] = getattr(self, name)
        if self.bc_coef is not None and "bc_coef" not in self.schedules:
            hp["bc_coef"] = self.bc_coef
        exchange = getattr(self, "exchange", None)
        if exchange is not None:  # `seed` above is already (seed + rank) mod 2^64
            hp.update(exchange_world=int(exchange.world), exchange_rank=int(exchange.rank))
        return hp

    def state_dict(self) -> dict:
        """The run state as CPU tensors and plain data: `weights`, `m`, `v`, `step`, `epochs_done`, the CPU generator's
        state (`generator`, its `get_state()` bytes), `progress_remaining`, the resolved `learning_rate` / `clip_range` /
        `clip_range_vf` (and `bc_coef` when it is set), `best_mean_reward`, `best_weights` and `episode_stats` (its state
        dict) when there are any, and
        `hyperparameters()`.  Schedules are callables and are not stored: construct the learner with them again."""
        from .checkpoint import cpu, generator_state

        sd = {"weights": cpu(self.weights), "m": cpu(self.m), "v": cpu(self.v), "step": int(self.step),
              "epochs_done": int(self.epochs_done), "generator": generator_state(self.generator),
              "progress_remaining": float(self.progress_remaining), "learning_rate": self.learning_rate,
              "clip_range": self.clip_range, "clip_range_vf": self.clip_range_vf,
              "best_mean_reward": float(self.best_mean_reward), "hyperparameters": self.hyperparameters()}
        if self.bc_coef is not None:
            sd["bc_coef"] = self.bc_coef
        if self.best_weights is not None:
            sd["best_weights"] = cpu(self.best_weights)
        if self.episode_stats is not None:
            sd["episode_stats"] = self.episode_stats.state_dict()
        return sd

    def check_state_dict(self, sd: dict, strict: bool = True) -> None:
        """ValueError, with nothing touched, unless `sd` can be loaded: the dims must match always; with strict=True every
        hyperparameter must (the message names every differing field with both values; a field scheduled on one side only
        shows under `scheduled` and as a value one side lacks)."""
        from .checkpoint import check_fingerprint, check_tensor

        saved, mine = dict(sd.get("hyperparameters") or {}), self.hyperparameters()
        check_fingerprint(saved, mine, "PPOLearner", fields=None if strict else ("obs_dim", "n_actions"))
        for key in ("weights", "m", "v") + (("best_weights",) if "best_weights" in sd else ()):
            check_tensor(sd, key, torch.empty(self.n_weights, dtype=torch.float32), "PPOLearner")
        if not isinstance(sd.get("generator"), torch.Tensor) or sd["generator"].dtype != torch.uint8 \
                or sd["generator"].shape != self.generator.get_state().shape:
            raise ValueError("PPOLearner: generator must be the byte tensor of a CPU generator's get_state()")
        for key in ("step", "epochs_done"):
            if isinstance(sd.get(key), bool) or not isinstance(sd.get(key), int) or sd[key] < 0:
                raise ValueError(f"PPOLearner: {key} must be a non-negative int, the checkpoint has {sd.get(key)!r}")
        if strict:
            for key in ("learning_rate", "clip_range", "clip_range_vf", "progress_remaining") + \
                    (("bc_coef",) if self.bc_coef is not None else ()):
                if key not in sd:
                    raise ValueError(f"PPOLearner: the checkpoint has no {key}")
        es = sd.get("episode_stats")
        if es is not None and self.episode_stats is not None and (self.episode_stats.num_envs, self.episode_stats.slots) == \
                (es.get("num_envs"), es.get("slots")):
            self.episode_stats.check_state_dict(es)

    def load_state_dict(self, sd: dict, strict: bool = True) -> None:
        """`check_state_dict`, then: the tensors are copied into the existing device tensors, the counters and the
        generator restored, `episode_stats` created if needed (dropped when the checkpoint has none), and the weights
        handed to the policy the way `update()` does it (`_hand_over()`, `policy.sync()`).
        strict=True: the stored `learning_rate` / `clip_range` / `clip_range_vf` come back as they were resolved.
        strict=False: only the dims must match and the constructor's values are kept - a changed learning rate, say -
        with this learner's schedules evaluated at the restored `progress_remaining`."""
        from .checkpoint import set_generator_state
        from .episodes import EpisodeStats

        self.check_state_dict(sd, strict=strict)
        es, stats = sd.get("episode_stats"), None
        if es is not None:  # first: a new EpisodeStats that refuses its part leaves the learner as it was
            stats = self.episode_stats
            if stats is None or (stats.num_envs, stats.slots) != (es.get("num_envs"), es.get("slots")):
                stats = EpisodeStats(es.get("num_envs"), self.device, slots=es.get("slots"))
            stats.load_state_dict(es)
        for key in ("weights", "m", "v"):
            getattr(self, key).copy_(sd[key])
        self.step, self.epochs_done = int(sd["step"]), int(sd["epochs_done"])
        set_generator_state(self.generator, sd["generator"])
        self.progress_remaining = float(sd.get("progress_remaining", 1.0))
        if strict:
            self.learning_rate, self.clip_range = float(sd["learning_rate"]), float(sd["clip_range"])
            self.clip_range_vf = None if sd["clip_range_vf"] is None else float(sd["clip_range_vf"])
            self.params.clip_range = self.clip_range
            if self.bc_coef is not None:
                self.bc_coef = float(sd["bc_coef"])
        else:
            self._resolve_schedules()
        self.best_mean_reward = float(sd.get("best_mean_reward", float("-inf")))
        if "best_weights" in sd:
            if self.best_weights is None:
                self.best_weights = torch.empty_like(self.weights)
            self.best_weights.copy_(sd["best_weights"])
        else:
            self.best_weights = None
        self.episode_stats = stats
        self._hand_over()
        self.policy.sync()

    def update(self, data: dict, progress_remaining: Optional[float] = None, explained_variance: bool = False) -> dict:
        """GAE, then n_epochs passes over a permutation of the K * N rows (shuffle="cpu": seeded on the CPU and copied to
        the device once per epoch; shuffle="device": one `mse_ppo_shuffle` launch per epoch; the last minibatch of an
        epoch may be short), one loss_grad + adam_step per minibatch without a host
        synchronisation, then the weights' hand-over to the policy (`weight_sync`).  Returns {"stats":
        f32[n_minibatches, 8] (device; columns STAT_NAMES), "mean": {name: float}}; with `bc_coef` set the columns are
        the twelve of PPO_BC_STAT_NAMES, and "mean" gains `bc_loss`, `bc_accuracy`, `bc_unusable`.
        With `target_kl` the result gains "stopped" (bool) and "minibatches_run" (int): "mean" is over the first
        minibatches_run rows of "stats", the rows after them stay zero.
        progress_remaining: sets `self.progress_remaining` first; the schedules are then evaluated once, here.
        explained_variance=True: one `mse_explained_variance` over the rollout's values / returns behind GAE and before
        the first minibatch; its f32 comes to the host in the copy that brings the statistics, and the result gains
        "explained_variance" (SB3's train/explained_variance; NaN when the returns are constant).
        With an `exchange`: `data` is this rank's rollout, `batch_size` counts rows per rank, a minibatch is the three phases
        with two all-reduces between them (class docstring), and "stats" / "mean" are those of the global minibatches,
        identical on every rank; explained_variance=True is refused (it would be this rank's rows only)."""
        if self.exchange is not None and explained_variance:
            raise ValueError("explained_variance cannot be combined with an exchange: it would cover this rank's rows only")
        if progress_remaining is not None:
            self.progress_remaining = float(progress_remaining)
        self._resolve_schedules()
        compute_gae(data, self.gamma, self.gae_lambda)
        K, n = data["rewards"].shape
        total = K * n
        bs = self.batch_size if self.batch_size is not None else (total + 3) // 4
        bs = max(1, min(int(bs), total))
        per_epoch = (total + bs - 1) // bs
        if self.exchange is not None:
            bs, plan = self._shard_plan(total)
            per_epoch = len(plan)
        n_mb = self.n_epochs * per_epoch
        gated = self.target_kl is not None
        names = STAT_NAMES if self.bc_coef is None else PPO_BC_STAT_NAMES[:11]
        w = 8 if self.bc_coef is None else 12  # columns of a minibatch's statistics
        ev = None
        if gated or explained_variance:  # statistics, control block and explained variance in one buffer: one copy brings all
            n_ctl, n_ev = (2 if gated else 0), (1 if explained_variance else 0)
            buf = torch.zeros(n_mb * w + n_ctl + n_ev, dtype=torch.float32, device=self.device)
            stats = buf[:n_mb * w].view(n_mb, w)
            control = buf[n_mb * w:n_mb * w + n_ctl].view(torch.int32) if gated else None
            if explained_variance:
                ev = buf[n_mb * w + n_ctl:]
                self.explained_variance(data, ev)
        else:
            stats, control = torch.zeros((n_mb, w), dtype=torch.float32, device=self.device), None
        step0 = self.step
        if self.exchange is not None:
            self._sharded_minibatches(data, total, bs, plan, stats, control)
        else:
            for i, rows in enumerate(self._minibatches(total, bs)):
                self.loss_grad(data, rows, rows.numel(), stats[i], control=control, target_kl=self.target_kl or 0.0)
                self.adam_step(control)
        self._hand_over()
        if not gated:
            if ev is None:
                mean = stats.mean(dim=0).cpu().tolist()
                self.policy.sync()
                return {"stats": stats, "mean": dict(zip(names, mean))}
            host = torch.cat((stats.mean(dim=0), ev)).cpu().tolist()  # still one copy
            self.policy.sync()
            return {"stats": stats, "mean": dict(zip(names, host[:w])), "explained_variance": host[w]}
        host = buf.cpu()
        self.policy.sync()
        stopped, run = (int(x) for x in host[n_mb * w:n_mb * w + 2].view(torch.int32))
        self.step = step0 + run - (1 if stopped else 0)  # the stopping minibatch took no step, nor did any after it
        mean = host[:n_mb * w].view(n_mb, w)[:run].mean(dim=0).tolist()
        out = {"stats": stats, "mean": dict(zip(names, mean)), "stopped": bool(stopped), "minibatches_run": run}
        if ev is not None:
            out["explained_variance"] = float(host[n_mb * w + 2])
        return out

    def learn(self, collector, iterations: int, callback=None, episode_stats: bool = False, eval_collector=None,
              eval_freq: int = 0, n_eval_episodes: int = 10, explained_variance: bool = False, first_iteration: int = 0,
              checkpoint_path=None, checkpoint_freq: int = 0, history: Optional[list] = None, check_sync: bool = False) -> list:
        """Alternates `collector.collect()` and `update()`; returns the per-iteration mean stats, each with the rollout's
        mean reward per env-step under "reward" (and, with `target_kl`, the update's "stopped" and "minibatches_run").
        episode_stats=True: each record gains `episodes`, `ep_rew_mean`, `ep_len_mean` over the episodes that ended in
        that iteration's rollout (NaN when none did); the running returns persist in `self.episode_stats` across
        iterations and across calls.
        eval_collector (a FusedPolicyRollout over this learner's policy and an env of its own) with eval_freq > 0: every
        eval_freq-th iteration gains `eval_mean_reward`, `eval_std_reward` from `evaluate_policy(eval_collector,
        n_eval_episodes)`; the best mean so far is kept in `best_mean_reward` with a device copy of the weights in
        `best_weights` (`restore_best()` loads them back).  With the defaults the records and the device work are
        what they were without these arguments.
        Before update `it` `progress_remaining` becomes `1 - (it + 1) / iterations`.  A record gains `learning_rate` and
        `clip_range` (the values that update used) when either is a schedule, `clip_range_vf` and `bc_coef` when set, and
        `explained_variance` with explained_variance=True.
        first_iteration: the loop runs `it` in range(first_iteration, iterations) with `progress_remaining` as above, so
        a run resumed from a checkpoint (`load_checkpoint`, then first_iteration = its "iteration") is on the same
        schedule and, bit for bit, the same run.  history: the records of the iterations already done (a checkpoint's
        "history"); the returned list then starts with them, else it holds the records of this call alone.
        checkpoint_freq > 0: after every checkpoint_freq-th iteration - the record appended, `callback` not yet called -
        `save_checkpoint(checkpoint_path, ...)` writes this learner, `collector` (with its env), the collector's frozen
        `sort_policy` if it has one (under policies["sort_policy"]), iteration = it + 1, `iterations` and the history so
        far; an `{iteration}` field in checkpoint_path is filled in, so earlier files can be kept.  `eval_collector`'s
        env is not saved and needs no state: `evaluate_policy` resets it every time.  With the defaults nothing is
        written and the loop is what it was.
        With an `exchange` every rank calls `learn` with its own collector; a checkpoint is per rank (give each rank its own
        checkpoint_path), explained_variance=True is refused, and check_sync=True adds `in_sync` to each record:
        `exchange.same_on_all_ranks(weights)`, off by default because it reads back."""
        if self.exchange is not None and explained_variance:
            raise ValueError("learn(explained_variance=True) cannot be combined with an exchange: it would cover this rank's "
                             "rows only")
        if check_sync and self.exchange is None:
            raise ValueError("check_sync needs an exchange")
        evaluate = self._evaluator(eval_collector, eval_freq, n_eval_episodes, keep_best=True)

        def step(data, progress_remaining):
            self.progress_remaining = progress_remaining
            out = self.update(data, explained_variance=True) if explained_variance else self.update(data)
            rec = dict(out["mean"], reward=float(data["rewards"].mean()))
            if "stopped" in out:  # target_kl is set
                rec.update(stopped=out["stopped"], minibatches_run=out["minibatches_run"])
            if "learning_rate" in self.schedules or "clip_range" in self.schedules:
                rec.update(learning_rate=self.learning_rate, clip_range=self.clip_range)
            if self.clip_range_vf is not None:
                rec.update(clip_range_vf=self.clip_range_vf)
            if self.bc_coef is not None:
                rec.update(bc_coef=self.bc_coef)
            if explained_variance:
                rec.update(explained_variance=out["explained_variance"])
            if check_sync:
                rec.update(in_sync=self.exchange.same_on_all_ranks(self.weights))
            return rec

        def checkpoint(iteration, history):
            sort_policy = getattr(collector, "sort_policy", None)
            save_checkpoint(format_path(checkpoint_path, iteration), learner=self, collector=collector,
                            policies=None if sort_policy is None else {"sort_policy": sort_policy}, iteration=iteration,
                            iterations=int(iterations), history=history)

        return training_loop(iterations, lambda it: collector.collect(), step, first_iteration=first_iteration, history=history,
                             stats_owner=self if episode_stats else None, stats_device=self.device, evaluate=evaluate,
                             eval_freq=eval_freq, checkpoint=None if checkpoint_path is None else checkpoint,
                             checkpoint_freq=checkpoint_freq, callback=callback)

    def _evaluator(self, eval_collector, eval_freq: int, n_eval_episodes: int, keep_best: bool = False):
        """`learn`'s evaluation: None unless eval_collector is given with eval_freq > 0 (one over another policy is refused),
        else a function -> `evaluate_policy(...)`'s pair that with keep_best also tracks `best_mean_reward` / `best_weights`."""
        if eval_collector is None or int(eval_freq) <= 0:
            return None
        if eval_collector.policy is not self.policy:
            raise ValueError("eval_collector must run this learner's policy")

        def evaluate():
            mean, std = evaluate_policy(eval_collector, n_eval_episodes=n_eval_episodes)
            if keep_best and mean > self.best_mean_reward:
                self.best_mean_reward = mean
                if self.best_weights is None:
                    self.best_weights = torch.empty_like(self.weights)
                self.best_weights.copy_(self.weights)  # device to device
            return mean, std

        return evaluate

    def restore_best(self) -> None:
        """Loads `best_weights` back into the learner's master copy and the policy (EvalCallback's best_model)."""
        if self.best_weights is None:
            raise RuntimeError("no evaluation has run: there are no best weights")
        self.weights.copy_(self.best_weights)
        self._hand_over()
        self.policy.sync()
