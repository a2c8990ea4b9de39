"""PARITY (GPU) at the batch sizes BASELINE.json names: every env, every step of the kernel the library picks at that
size, against the batched CPU oracle (oracle.OracleBatch) - not against another HIP kernel.

The library chooses its rollout kernel by batch size relative to the CU count (mse_create, launch_rollout_policy), so
the sizes here are multiples of the device's CU count: on an MI355X (256 CUs) they are 65 536, 65 537, 131 072 and
262 144.  Each case forces the kernel by rollout_pipeline where the library allows it, and names it.

Random-policy and step paths: the recorded actions replay through the oracle; each must be the masked-uniform draw of
the host restatement of the policy stream (tests/policy_stream.py) over the ORACLE's pre-step mask; observations bit
for bit; masks and done exact; the f32 reward within max(1e-6, 2**-24 |r|) of the oracle's f64 reward and equal to it
rounded to f32 (the kernels store (float) of their f64 reward); the full state after each launch.

Learned-policy path (FusedPolicyRollout): the same dynamics check, plus the network restated in torch float64
(F.linear, tanh, log_softmax over logits masked to -1e8) on the recorded observations and masks of every row."""
import numpy as np
import pytest

from oracle.oracle import SNAP, OracleBatch
from tests import policy_stream as ps

pytestmark = pytest.mark.gpu

MAX_STEPS = 25
LAUNCHES = (20, 20, 7, 64, 1, 16)  # >= 16 steps (the ring's two-half priming), short launches, resets everywhere
STATE_COLS = ("input", "belt", "sorting", "cont_true", "cont_false", "cont_e", "press_timer", "press_mat", "press_n",
              "press_q100", "mode", "last_press_started", "last_press_amount", "current_step", "gen_first", "gen_idx",
              "gen_counter", "bale_count", "bale_sum", "bale_last_size", "bale_last_q", "episode")
_COL_IDX = np.concatenate([np.arange(SNAP[c].start, SNAP[c].stop) for c in STATE_COLS])
_COL_NAME = [c for c in STATE_COLS for _ in range(SNAP[c].stop - SNAP[c].start)]
LOGP_TOL, VALUE_ATOL, VALUE_RTOL = 1e-4, 2e-5, 1e-6


def _cus():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


def _mk(kind, n, **kw):
    import marl_sortingenv_amd as M

    return M.BatchedSortingEnv(kind=kind, num_envs=n, device=0, balesize=200, auto_reset=True, **kw)


def _np(t):
    return t.cpu().numpy()


def _same(tag, got, exp):
    """got == exp row by row (bitwise for floats); the message names the first env that differs."""
    got, exp = np.asarray(got), np.asarray(exp)
    if got.dtype.kind == "f":
        got, exp = got.view(np.uint32 if got.itemsize == 4 else np.uint64), exp.view(np.uint32 if exp.itemsize == 4 else np.uint64)
    neq = got != exp
    if neq.ndim > 1:
        neq = neq.any(axis=tuple(range(1, neq.ndim)))
    bad = np.flatnonzero(neq)
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f"{tag}: {bad.size} envs differ, first env {i}: got {np.asarray(got[i]).tolist()} "
                             f"expected {np.asarray(exp[i]).tolist()}")


def _check_reward(tag, rew32, r64):
    """The f32 reward buffer against the oracle's f64 reward: within max(1e-6, 2**-24 |r|), and the nearest f32 to it
    (the kernels store (float) of their own f64 reward, which differs from the oracle's only in tanh's last bits)."""
    rew32 = np.asarray(rew32, dtype=np.float32)
    err = np.abs(rew32.astype(np.float64) - r64)
    bad = np.flatnonzero(err > np.maximum(1e-6, 2.0 ** -24 * np.abs(r64)))
    assert bad.size == 0, f"{tag}: reward of env {int(bad[0])}: {float(rew32[bad[0]])!r} vs {float(r64[bad[0]])!r}"
    half_ulp = 0.5 * np.spacing(np.abs(rew32)).astype(np.float64)
    bad = np.flatnonzero(err > half_ulp + 1e-9 * np.abs(r64) + 1e-12)
    assert bad.size == 0, f"{tag}: f32 reward of env {int(bad[0])} is not its f64 reward rounded: " \
                          f"{float(rew32[bad[0]])!r} vs {float(r64[bad[0]])!r}"


def _check_state(tag, env, orc, noise, words=None):
    """The engine's state (mse_get_state) against the oracle's snapshot for all N envs: the integer columns of
    tests/test_gpu_batched.py's _compare_state, the accuracies, and the PCG64 words of rng, rng_pressing (with its
    buffered half) and rng_sorting - rng_noise as well when noise is on (with noise 0 it is never advanced)."""
    ints, dbls, rng = env.get_state()
    ints, dbls, rng = _np(ints), _np(dbls), _np(rng).view(np.uint64)
    I, D, R = orc.snapshot()
    neq = ints[:, _COL_IDX] != I[:, _COL_IDX]
    bad = np.flatnonzero(neq.any(axis=1))
    if bad.size:
        i = int(bad[0])
        cols = sorted({_COL_NAME[c] for c in np.flatnonzero(neq[i])})
        raise AssertionError(f"{tag}: state of {bad.size} envs differs, first env {i} in {cols}: "
                             f"{ints[i, _COL_IDX][neq[i]].tolist()} vs {I[i, _COL_IDX][neq[i]].tolist()}")
    _same(f"{tag}: accuracies", dbls, np.ascontiguousarray(D[:, :4]))
    if words is None:
        words = list(range(0, 4)) + list(range(12, 24)) + (list(range(6, 10)) if noise else [])
    _same(f"{tag}: PCG64 words {words}", rng[:, words], R[:, words])


def _frozen_sorter(n):
    """bench.py's frozen Bernoulli(1/2) sorting decisions for Env_2 (Workload, rank 0)."""
    import torch

    g = torch.Generator(device="cpu").manual_seed(1234)
    return (torch.rand(n, generator=g) < 0.5).to(torch.int32)


def _start(tag, env, orc, noise):
    _same(f"{tag}: reset obs", _np(env.obs), orc.obs())
    _same(f"{tag}: reset mask", _np(env.mask), orc.action_masks())
    _check_state(f"{tag}: after reset", env, orc, noise)


def _run_rollouts(tag, env, orc, noise, launches, policy_seed, sort_mode=None, hows=None):
    """mse_rollout launches of the given lengths; every step of every env replayed through the oracle."""
    n = env.num_envs
    key = ps.policy_key(policy_seed, np.arange(n, dtype=np.uint64) + np.uint64(env.index_offset))
    sm_dev = None if sort_mode is None else sort_mode.cuda()
    sm = None if sort_mode is None else sort_mode.numpy()
    buf = env.alloc_rollout(max(launches))
    t = env.policy_step
    for li, K in enumerate(launches):
        how = (hows or {}).get(li, {})
        masked = how.get("use_action_masking", True)
        env.rollout(K, policy_seed=policy_seed, buffers=buf, sort_mode=sm_dev, **how)
        acts, rews, dones = _np(buf["actions"][:K]), _np(buf["reward"][:K]), _np(buf["done"][:K])
        ohow = dict(how, sanitize_late=not masked and env.kind == "mono")
        for k in range(K):
            at = f"{tag} launch {li} (K={K}) step {k}"
            out = orc.step(acts[k], sort_mode=sm, **ohow)
            _same(f"{at}: action vs the host stream's draw", acts[k],
                  ps.masked_uniform(ps.policy_word(key, t), out["mask_pre"], masked))
            _same(f"{at}: obs", _np(buf["obs"][k]), out["obs"])
            _same(f"{at}: mask", _np(buf["mask"][k]), out["mask"])
            _same(f"{at}: done", dones[k], out["term"])
            _check_reward(at, rews[k], out["reward"])
            t += 1
        _check_state(f"{tag} after launch {li}", env, orc, noise)
    assert env.policy_step == t
    assert env.error_count() == 0


# ---- random policy: mse_rollout ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("noise", [0.0, 0.05])
def test_R1_ring_one_round(noise):
    """R1: 256 x CUs envs (65 536 on an MI355X), Env_3: k_rollout_ring, one round of workgroups (rollout_pipeline 3)."""
    n = 256 * _cus()
    env = _mk("mono", n, base_seed=0, max_steps=MAX_STEPS, noise_sorting=noise, rollout_pipeline=3)
    orc = OracleBatch("mono", n, base_seed=0, max_steps=MAX_STEPS, noise_sorting=noise)
    _start("R1", env, orc, noise)
    _run_rollouts(f"R1 noise={noise}", env, orc, noise, LAUNCHES, policy_seed=2024)


@pytest.mark.parametrize("kind", ["press", "sort"])
def test_R2_ring_press_and_sort(kind):
    """R2: 256 x CUs envs: k_rollout_ring KIND 2 (Env_2 with bench.py's frozen Bernoulli(1/2) sorter) and KIND 1."""
    n = 256 * _cus()
    sm = _frozen_sorter(n) if kind == "press" else None
    env = _mk(kind, n, base_seed=0, max_steps=MAX_STEPS, noise_sorting=0.0, rollout_pipeline=3)
    orc = OracleBatch(kind, n, base_seed=0, max_steps=MAX_STEPS, noise_sorting=0.0)
    _start("R2", env, orc, 0.0)
    _run_rollouts(f"R2 {kind}", env, orc, 0.0, LAUNCHES, policy_seed=2024, sort_mode=sm)


def test_R3_ring_two_rounds():
    """R3: 512 x CUs envs (131 072): k_rollout_ring over two rounds of workgroups (workgroup index >= CUs)."""
    n = 512 * _cus()
    env = _mk("mono", n, base_seed=0, max_steps=MAX_STEPS, noise_sorting=0.0, rollout_pipeline=3)
    orc = OracleBatch("mono", n, base_seed=0, max_steps=MAX_STEPS, noise_sorting=0.0)
    _start("R3", env, orc, 0.0)
    _run_rollouts("R3", env, orc, 0.0, LAUNCHES, policy_seed=2024)


def test_R4_dynamics_observer_kernel():
    """R4: 256 x CUs envs, rollout_pipeline 1: k_rollout_po (dynamics / observer waves, no RNG waves)."""
    n = 256 * _cus()
    env = _mk("mono", n, base_seed=0, max_steps=MAX_STEPS, noise_sorting=0.05, rollout_pipeline=1)
    orc = OracleBatch("mono", n, base_seed=0, max_steps=MAX_STEPS, noise_sorting=0.05)
    _start("R4", env, orc, 0.05)
    _run_rollouts("R4", env, orc, 0.05, LAUNCHES, policy_seed=99)


def test_R5_one_lane_ragged_last_workgroup():
    """R5: 256 x CUs + 1 envs (65 537): k_rollout, one lane per env (the size rule's choice; rollout_pipeline 2 forces
    it), whose last workgroup holds a single env."""
    n = 256 * _cus() + 1
    env = _mk("mono", n, base_seed=0, max_steps=MAX_STEPS, noise_sorting=0.0, rollout_pipeline=2)
    orc = OracleBatch("mono", n, base_seed=0, max_steps=MAX_STEPS, noise_sorting=0.0)
    _start("R5", env, orc, 0.0)
    _run_rollouts("R5", env, orc, 0.0, LAUNCHES, policy_seed=2024)


def test_R6_one_lane_full_size_with_flags():
    """R6: 1024 x CUs envs (262 144, BASELINE configs[3]): k_rollout; one launch unmasked (the reference's mode='random'
    sequencing: sanitize late), one with check_overflow."""
    n = 1024 * _cus()
    env = _mk("mono", n, base_seed=0, max_steps=MAX_STEPS, noise_sorting=0.05, rollout_pipeline=2)
    orc = OracleBatch("mono", n, base_seed=0, max_steps=MAX_STEPS, noise_sorting=0.05)
    _start("R6", env, orc, 0.05)
    hows = {2: dict(use_action_masking=False), 5: dict(check_overflow=True)}
    _run_rollouts("R6", env, orc, 0.05, LAUNCHES, policy_seed=2024, hows=hows)


def test_R7_one_lane_last_rank_index_offset():
    """R7: 1024 x CUs envs at index_offset 7 x 1024 x CUs: BASELINE configs[4]'s last rank on one GPU, k_rollout; env
    seeds and policy keys come from the global index."""
    n = 1024 * _cus()
    off = 7 * n
    env = _mk("mono", n, base_seed=0, index_offset=off, max_steps=MAX_STEPS, noise_sorting=0.0, rollout_pipeline=2)
    orc = OracleBatch("mono", n, base_seed=off, max_steps=MAX_STEPS, noise_sorting=0.0)
    _start("R7", env, orc, 0.0)
    _run_rollouts("R7", env, orc, 0.0, (20, 7, 1, 16), policy_seed=2024)


# ---- the step path: k_sample + k_step -------------------------------------------------------------------------------

def _run_steps(tag, env, orc, noise, steps, policy_seed):
    """sample_actions + step(want_reward64, want_terminal_obs), replayed through the oracle every step."""
    n = env.num_envs
    key = ps.policy_key(policy_seed, np.arange(n, dtype=np.uint64) + np.uint64(env.index_offset))
    for s in range(steps):
        at = f"{tag} step {s}"
        t = env.policy_step
        act = env.sample_actions(policy_seed=policy_seed)
        obs, rew, done, mask = env.step(act, want_reward64=True, want_terminal_obs=True)
        out = orc.step(_np(act), want_terminal_obs=True)
        _same(f"{at}: action vs the host stream's draw", _np(act), ps.masked_uniform(ps.policy_word(key, t), out["mask_pre"]))
        _same(f"{at}: obs", _np(obs), out["obs"])
        _same(f"{at}: mask", _np(mask), out["mask"])
        d = _np(done)
        _same(f"{at}: done", d, out["term"])
        r64 = _np(env.reward64)
        bad = np.flatnonzero(np.abs(r64 - out["reward"]) > 1e-6)
        assert bad.size == 0, f"{at}: reward64 of env {int(bad[0])}: {r64[bad[0]]!r} vs {out['reward'][bad[0]]!r}"
        _check_reward(at, _np(rew), out["reward"])
        ended = np.flatnonzero(d)
        _same(f"{at}: terminal obs", _np(env.terminal_obs)[ended], out["terminal_obs"][ended])
        if s % 10 == 9 or s == steps - 1:
            _check_state(at, env, orc, noise)
    assert env.error_count() == 0


def test_S1_step_path():
    """S1: 256 x CUs envs, ~30 single steps: k_sample + k_step (bench.py --mode step), reward64 and terminal obs."""
    n = 256 * _cus()
    env = _mk("mono", n, base_seed=0, max_steps=MAX_STEPS, noise_sorting=0.05)
    orc = OracleBatch("mono", n, base_seed=0, max_steps=MAX_STEPS, noise_sorting=0.05)
    _start("S1", env, orc, 0.05)
    _run_steps("S1", env, orc, 0.05, 30, policy_seed=7)


# ---- large seeds on the device ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("base_seed,policy_seed", [(2**32 - 2048, 2**40 + 7), (2**63 - 5000, 2**64 - 1)])
def test_L1_large_seeds(base_seed, policy_seed):
    """L1: 4 096 envs seeded across 2**32 and just below 2**63, policy seeds with a high word: the device SeedSequence's
    high entropy word and the policy key's seed >> 32 term.  Rollout and step paths, then a partial reset(seeds=...)
    with 0, 2**32 - 1, 2**32 and 2**63 - 1."""
    import torch

    n, noise = 4096, 0.05
    env = _mk("mono", n, base_seed=base_seed, max_steps=MAX_STEPS, noise_sorting=noise)
    orc = OracleBatch("mono", n, base_seed=base_seed, max_steps=MAX_STEPS, noise_sorting=noise)
    _start("L1", env, orc, noise)
    _check_state("L1: after reset, every stream", env, orc, noise, words=list(range(0, 4)) + list(range(6, 10)) + list(range(12, 30)))
    _run_rollouts("L1", env, orc, noise, (20, 7), policy_seed=policy_seed)
    _run_steps("L1", env, orc, noise, 6, policy_seed=policy_seed)
    which = (np.arange(n) % 5 == 0).astype(np.uint8)
    seeds = np.array([0, 2**32 - 1, 2**32, 2**63 - 1], dtype=np.uint64)[(np.arange(n) // 5) % 4]
    obs, mask = env.reset(seeds=torch.from_numpy(seeds.astype(np.int64)), which=torch.from_numpy(which))
    exp = orc.reset(seeds=seeds, which=which)
    _same("L1: partial reset obs", _np(obs), exp)
    _same("L1: partial reset mask", _np(mask), orc.action_masks())
    _check_state("L1: after the partial reset", env, orc, noise)
    ints, _, rng = env.get_state()
    I, _, R = orc.snapshot()
    sel = np.flatnonzero(which)
    _same("L1: reset envs' generator stream", _np(rng).view(np.uint64)[sel, 24:30], R[sel, 24:30])
    _run_rollouts("L1 after reset", env, orc, noise, (16,), policy_seed=policy_seed)


# ---- learned policy: mse_rollout_policy, oracle + fp64 network ------------------------------------------------------

def _policy(obs_dim, n_actions, head_gain, precision):
    """MlpPolicy.random_init (SB3's initial scale: action head gain 0.01, near-uniform softmax), or the same weights
    with the action head at gain 1 (a sharper, trained-like softmax).  Returns (policy, float64 weights on the GPU)."""
    import torch

    import marl_sortingenv_amd as M
    from marl_sortingenv_amd.policy import SB3_KEYS, _shapes

    base = M.MlpPolicy.random_init(obs_dim, n_actions, seed=7, device=0, precision=precision)
    w = {k: base.weights[k].reshape(s) for k, s in zip(SB3_KEYS, _shapes(obs_dim, n_actions))}
    if head_gain != 0.01:
        w["action_net.weight"] = (w["action_net.weight"] * np.float32(head_gain / 0.01)).astype(np.float32)
    pol = M.MlpPolicy(obs_dim, n_actions, w, device=0, precision=precision)
    assert pol.precision == precision
    return pol, {k: torch.from_numpy(v.astype(np.float64)).cuda() for k, v in w.items()}


def _net64(w, obs, mask):
    """The reference's policy in float64 (MaskableActorCriticPolicy; sb3_contrib masks logits to -1e8)."""
    import torch
    import torch.nn.functional as F

    def mlp(x, net):
        x = torch.tanh(F.linear(x, w[f"mlp_extractor.{net}.0.weight"], w[f"mlp_extractor.{net}.0.bias"]))
        return torch.tanh(F.linear(x, w[f"mlp_extractor.{net}.2.weight"], w[f"mlp_extractor.{net}.2.bias"]))

    obs = obs.double()
    logits = F.linear(mlp(obs, "policy_net"), w["action_net.weight"], w["action_net.bias"])
    logits = torch.where(mask.bool(), logits, torch.full_like(logits, -1e8))
    value = F.linear(mlp(obs, "value_net"), w["value_net.weight"], w["value_net.bias"]).squeeze(1)
    return logits, torch.log_softmax(logits, dim=1), value


def _register_order(n_actions):
    """The order the kernels accumulate the softmax masses in (the MFMA accumulator's rows, csrc/mse_policy_device.h)."""
    return [a for h in (0, 1) for r in range(16) for a in [(r & 3) + 8 * (r >> 2) + 4 * h] if a < n_actions]


def _check_values(tag, got, ref):
    import torch

    err = (got.double() - ref).abs()
    bad = torch.nonzero(err > VALUE_ATOL + VALUE_RTOL * ref.abs()).flatten()
    assert bad.numel() == 0, f"{tag}: value of env {int(bad[0])}: {float(got[bad[0]])!r} vs {float(ref[bad[0]])!r}"


def _run_policy_collect(tag, col, orc, noise, w64, deterministic, prev_done, counts):
    """One FusedPolicyRollout.collect; dynamics replayed through the oracle, the network checked in float64."""
    import torch

    env = col.env
    n, A, K = env.num_envs, env.num_actions, col.n_steps
    order = torch.tensor(_register_order(A), device="cuda")
    key = ps.policy_key(col.seed, np.arange(n, dtype=np.uint64) + np.uint64(env.index_offset))
    sm = None if col.sort_mode is None else _np(col.sort_mode)
    t0 = env.policy_step
    b = col.collect(deterministic=deterministic)
    assert env.policy_step == t0 + K
    for k in range(K):
        at = f"{tag} step {k}"
        obs_k, mask_k = b["observations"][k], b["action_masks"][k]
        act = b["actions"][k]
        _same(f"{at}: observation", _np(obs_k), orc.obs())
        _same(f"{at}: action mask", _np(mask_k), orc.action_masks())
        _same(f"{at}: episode start", _np(b["episode_starts"][k]), prev_done)
        logits, logsm, value = _net64(w64, obs_k, mask_k)
        a_l = act.long().unsqueeze(1)
        assert bool(((act >= 0) & (act < A)).all()), at
        assert bool(mask_k.bool().gather(1, a_l).all()), f"{at}: a masked action was taken"
        lp_err = (b["log_probs"][k].double() - logsm.gather(1, a_l).squeeze(1)).abs()
        assert float(lp_err.max()) <= LOGP_TOL, (at, float(lp_err.max()), int(lp_err.argmax()))
        _check_values(at, b["values"][k], value)
        if deterministic:
            top2 = torch.topk(logits, 2, dim=1).values
            clear = (top2[:, 0] - top2[:, 1]) > 1e-4
            wrong = torch.nonzero(clear & (act.long() != logits.argmax(dim=1))).flatten()
            assert wrong.numel() == 0, f"{at}: deterministic action of env {int(wrong[0])} is not the fp64 argmax"
        else:
            # the inverse cdf of the stream's u = (w >> 8) 2**-24 over the softmax masses in register order, in fp64
            u = torch.from_numpy(ps.uniform24(ps.policy_word(key, t0 + k))).cuda()
            cdf = torch.cumsum(torch.softmax(logits, dim=1)[:, order], dim=1)
            j = torch.searchsorted(cdf, u.unsqueeze(1), right=True).squeeze(1).clamp_(max=A - 1)
            miss = torch.nonzero(order[j] != act.long()).flatten()
            if miss.numel():
                near = (cdf[miss] - u[miss].unsqueeze(1)).abs().min(dim=1).values
                assert float(near.max()) < 1e-5, f"{at}: env {int(miss[int(near.argmax())])} sampled off the cdf"
            counts[0] += int(miss.numel())
            counts[1] += n
        out = orc.step(_np(act), sort_mode=sm)
        _check_reward(at, _np(b["rewards"][k]), out["reward"])
        prev_done = out["term"]
    _same(f"{tag}: last dones", _np(b["last_dones"]), prev_done)
    obs_end = torch.from_numpy(orc.obs()).cuda()
    _, _, v_end = _net64(w64, obs_end, torch.from_numpy(orc.action_masks()).cuda())
    _check_values(f"{tag}: last values", b["last_values"], v_end)
    _check_state(f"{tag}: state after the collect", env, orc, noise)
    return prev_done


def _run_policy_case(tag, kind, n, noise, precision, head_gain, K=16, pipeline=0):
    import marl_sortingenv_amd as M

    env = _mk(kind, n, base_seed=0, max_steps=MAX_STEPS, noise_sorting=noise, rollout_pipeline=pipeline)
    orc = OracleBatch(kind, n, base_seed=0, max_steps=MAX_STEPS, noise_sorting=noise)
    _start(tag, env, orc, noise)
    pol, w64 = _policy(env.obs_dim, env.num_actions, head_gain, precision)
    sm = _frozen_sorter(n).cuda() if kind == "press" else None
    col = M.FusedPolicyRollout(env, pol, K, seed=5, sort_mode=sm)
    prev_done, counts = np.ones(n, dtype=np.uint8), [0, 0]
    for it in range(2):
        prev_done = _run_policy_collect(f"{tag} collect {it}", col, orc, noise, w64, False, prev_done, counts)
    prev_done = _run_policy_collect(f"{tag} deterministic collect", col, orc, noise, w64, True, prev_done, counts)
    assert counts[0] <= 1e-4 * counts[1], f"{tag}: {counts[0]} of {counts[1]} sampled actions off the fp64 inverse cdf"
    assert env.error_count() == 0


HEADS = [pytest.param(0.01, id="sb3init"), pytest.param(1.0, id="gain1")]


@pytest.mark.parametrize("head_gain", HEADS)
@pytest.mark.parametrize("noise", [0.0, 0.05])
def test_P1_policy_roles_mono(noise, head_gain):
    """P1: 256 x CUs envs, Env_3, f16x3: k_rollout_policy_roles with RNG waves."""
    _run_policy_case("P1", "mono", 256 * _cus(), noise, "f16x3", head_gain)


@pytest.mark.parametrize("head_gain", HEADS)
@pytest.mark.parametrize("kind", ["press", "sort"])
def test_P2_policy_roles_press_and_sort(kind, head_gain):
    """P2: 256 x CUs envs, f16x3: k_rollout_policy_roles KIND 2 (bench.py's frozen sort_mode tensor) and KIND 1."""
    _run_policy_case("P2", kind, 256 * _cus(), 0.05, "f16x3", head_gain)


@pytest.mark.parametrize("head_gain", HEADS)
def test_P3_policy_two_tiles_f16x3(head_gain):
    """P3: 1024 x CUs envs (262 144, BASELINE configs[3]), Env_3, f16x3, K = 16: k_rollout_policy<3, ., 2, true>."""
    _run_policy_case("P3", "mono", 1024 * _cus(), 0.0, "f16x3", head_gain)


@pytest.mark.parametrize("head_gain", HEADS)
@pytest.mark.parametrize("per_cu", [1024, 256])
def test_P4_policy_exact_f32(per_cu, head_gain):
    """P4: Env_3, exact f32 form: k_rollout_policy TILES=2 with 8 waves per workgroup (1024 x CUs envs) and with 4
    (256 x CUs)."""
    _run_policy_case("P4", "mono", per_cu * _cus(), 0.05, "f32", head_gain)
