"""GPU: the modular collection in Env_3 (mse_rollout_modular, FusedModularRollout) - the sorting agent (13 -> 2) and the
pressing agent (16 -> 11) sampling side by side inside one rollout kernel - against

  * its multi-launch twin ModularRolloutCollector (previews, two MlpPolicy forwards, mse_step): bit for bit, every
    buffer the twin fills, the full state and the policy step counter after every launch, at both wave shapes;
  * per-env oracle.OracleEnv replays of the recorded flat actions: previews, press masks, dones, the reward and its two
    parts (the oracle's trace record);
  * the float64 restatement of both networks and the bit-exact float32 sampler on zero-head agents;
  * the shipped k_rollout_model when both agents are deterministic;
  * guard words, NULL outputs, the untouched rng_sorting / rng_pressing streams, and its refusals, one status each.

All envs run max_steps=3, so episodes end inside and across launches."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle.oracle import OracleEnv
from tests import policy_head_reference as R
from tests import policy_stream as ps
from tests import replay
from tests.rollout_checks import OVERFLOW_OVERRIDES, bits_equal, cus, guarded, inside, overflow_config
from tests.test_gpu_full_size_oracle import _check_reward, _same
from tests.test_gpu_model_rollout import _agents, _state_equal

pytestmark = pytest.mark.gpu

MAX_STEPS = 3
SORT_SEED, PRESS_SEED = 2024, 2025
TWIN_KEYS = ("sort_obs", "press_obs", "press_masks", "episode_starts", "sort_actions", "press_actions", "sort_log_probs",
             "press_log_probs", "sort_values", "press_values", "rewards", "sort_last_values", "press_last_values",
             "last_dones")
# MSE_TRACE_* columns of include/mse.h
TRACE_R_SORT, TRACE_R_PRESS, TRACE_REWARD, TRACE_OVERFLOW = 1, 2, 32, 37
# at this capacity (config.yml: 700) a container overflows in the third step of every episode the CPU oracle was
# tried on, whatever the actions
OVERFLOW_META = dict(kind="mono", max_steps=MAX_STEPS, noise_sorting=0.0, balesize=200, config_overrides=OVERFLOW_OVERRIDES)


def _env(n, noise, base_seed=0, **kw):
    import marl_sortingenv_amd as M

    kw.setdefault("auto_reset", True)
    kw.setdefault("max_steps", MAX_STEPS)
    env = M.BatchedSortingEnv(kind="mono", num_envs=n, device=0, base_seed=base_seed, noise_sorting=noise, balesize=200, **kw)
    assert env._cfg_struct.noise == noise  # the constructor's noise_sorting is what the handle runs at, whatever `config` says
    return env


@functools.lru_cache(maxsize=None)
def _pair(seed=0, head_gain=20.0):
    """The two agents in the f16x3 form, the action heads scaled up so that the draws matter; built once and shared
    (no test changes their weights)."""
    sort_ag, press_ag, _ = _agents("both_maskable", seed=seed, head_gain=head_gain)
    return sort_ag, press_ag


def _dones(b, K):
    """u8[K, N]: step k ended an episode, from the next row's episode start and last_dones."""
    import torch

    return torch.cat([b["episode_starts"][1:K], b["last_dones"][None]]).cpu().numpy() != 0


def _overflow_ends(b, K, dones):
    """Rows that ended an episode by overflow, as the buffers show them: the reward is the overflow termination penalty
    itself and both parts are half of it (env_monolith.py:271); no other step's reward comes near it."""
    from marl_sortingenv_amd.config import SortingEnvConfig

    pen = np.float32(SortingEnvConfig().overflow_termination_penalty)
    rew, rs, rp = (b[k][:K].cpu().numpy() for k in ("rewards", "rewards_sort", "rewards_press"))
    hit = rew == pen
    assert (dones[hit]).all() and (rs[hit] == pen / 2).all() and (rp[hit] == pen / 2).all()
    assert (rew[~hit] > pen / 2).all()
    return int(hit.sum())


# ---- 1. fused == twin, bit for bit ------------------------------------------------------------------------------------
MODES = {
    "sampled": dict(),
    "sort_det": dict(sort_deterministic=True),
    "press_det": dict(press_deterministic=True),
    "both_det": dict(sort_deterministic=True, press_deterministic=True),
    "overflow": dict(check_overflow=True),
}


def _compare_with_twin(tag, n, noise, press_masked, mode, launches, config=None, base_seed=11, **kw):
    import marl_sortingenv_amd as M

    sort_ag, press_ag = _pair()
    if config is not None:
        kw["config"] = config
    a, b = _env(n, noise, base_seed=base_seed, **kw), _env(n, noise, base_seed=base_seed, **kw)
    kmax = max(launches)
    fused = M.FusedModularRollout(a, sort_ag, press_ag, kmax, SORT_SEED, PRESS_SEED, press_masked=press_masked)
    twin = M.ModularRolloutCollector(b, sort_ag, press_ag, kmax, SORT_SEED, PRESS_SEED, press_masked=press_masked)
    n_done = n_early = 0  # n_early: episodes ended by overflow
    for K in launches:
        t0 = a.policy_step
        got, exp = fused.collect(K, **MODES[mode]), twin.collect(K, **MODES[mode])
        bits_equal(f"{tag} K={K}", got, exp, TWIN_KEYS, K)
        _state_equal(f"{tag} K={K}", a, b)
        assert a.policy_step == t0 + K
        dones = _dones(got, K)
        n_done += int(dones.sum())
        n_early += _overflow_ends(got, K, dones)
    a.close()
    b.close()
    return n_done, n_early


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("press_masked", [True, False], ids=["masked", "plain"])
@pytest.mark.parametrize("noise", [0.0, 0.05], ids=["n0", "n5"])
@pytest.mark.parametrize("n", [1, 33, 257])
def test_fused_modular_rollout_matches_twin(n, noise, press_masked, mode):
    """A lone lane, a ragged second tile, a second workgroup with one env; launches of 5, 1 and 4 steps on the same
    handles."""
    config = overflow_config(noise) if mode == "overflow" else None
    n_done, n_early = _compare_with_twin(f"n={n} noise={noise} masked={press_masked} {mode}", n, noise, press_masked, mode,
                                         (5, 1, 4), config=config)
    assert n_done >= 2 * n
    if mode == "overflow":
        assert n_early >= 1, "no episode ended by overflow"
    else:
        assert n_early == 0


# ---- 2. the second wave shape ----------------------------------------------------------------------------------------
def test_fused_modular_rollout_matches_twin_in_64_env_waves():
    """256 x CUs + 1 envs: the smallest batch plan_policy_plain gives two tiles per wave."""
    _compare_with_twin("tiles=2", 256 * cus() + 1, 0.05, True, "sampled", (2,))


# ---- 3. the oracle ---------------------------------------------------------------------------------------------------
def test_fused_modular_rollout_matches_oracle():
    import marl_sortingenv_amd as M

    n, K, base, noise = 33, 6, 700, 0.05
    sort_ag, press_ag = _pair()
    env = _env(n, noise, base_seed=base)
    orcs = [OracleEnv(kind="mono", max_steps=MAX_STEPS, seed=base + i, noise_sorting=noise) for i in range(n)]
    for i, o in enumerate(orcs):
        o.reset(base + i)
    b = M.FusedModularRollout(env, sort_ag, press_ag, K, SORT_SEED, PRESS_SEED).collect()
    rows = {k: v.cpu().numpy() for k, v in b.items()}
    dones = _dones(b, K)
    flat = 11 * rows["sort_actions"] + rows["press_actions"]
    for k in range(K):
        for j, o in enumerate(orcs):
            at = f"step {k} env {j}"
            _same(f"{at}: sort_obs", rows["sort_obs"][k, j][None], o.sort_agent_obs()[None])
            _same(f"{at}: press_obs", rows["press_obs"][k, j][None], o.press_agent_obs()[None])
            _same(f"{at}: press_masks", rows["press_masks"][k, j][None], o.action_masks()[:11].astype(np.uint8)[None])
            _, r64, term = o.step(int(flat[k, j]), check_overflow=False)
            rec = o.trace_record()
            assert rec[TRACE_REWARD] == r64
            _check_reward(f"{at}: rewards", rows["rewards"][k, j:j + 1], rec[TRACE_REWARD:TRACE_REWARD + 1])
            _check_reward(f"{at}: rewards_sort", rows["rewards_sort"][k, j:j + 1], rec[TRACE_R_SORT:TRACE_R_SORT + 1])
            _check_reward(f"{at}: rewards_press", rows["rewards_press"][k, j:j + 1], rec[TRACE_R_PRESS:TRACE_R_PRESS + 1])
            assert bool(dones[k, j]) == bool(term), at
            if term:
                o.reset(None)
    assert dones.sum() >= n
    env.close()


def test_fused_modular_rollout_overflow_parts_match_oracle():
    """check_overflow: an overflow termination is seen by the oracle's trace record, and both parts are reward / 2."""
    import marl_sortingenv_amd as M

    n, K, base = 33, 6, 40
    sort_ag, press_ag = _pair()
    env = _env(n, 0.0, base_seed=base, config=overflow_config(0.0))
    orcs = [OracleEnv(kind="mono", seed=base + i, cfg=replay.oracle_config(OVERFLOW_META)) for i in range(n)]
    for i, o in enumerate(orcs):
        o.reset(base + i)
    b = M.FusedModularRollout(env, sort_ag, press_ag, K, SORT_SEED, PRESS_SEED).collect(check_overflow=True)
    rows = {k: v.cpu().numpy() for k, v in b.items()}
    dones = _dones(b, K)
    flat = 11 * rows["sort_actions"] + rows["press_actions"]
    overflows = 0
    for k in range(K):
        for j, o in enumerate(orcs):
            at = f"step {k} env {j}"
            _, r64, term = o.step(int(flat[k, j]), check_overflow=True)
            rec = o.trace_record()
            for key, col in (("rewards", TRACE_REWARD), ("rewards_sort", TRACE_R_SORT), ("rewards_press", TRACE_R_PRESS)):
                _check_reward(f"{at}: {key}", rows[key][k, j:j + 1], rec[col:col + 1])
            assert bool(dones[k, j]) == bool(term), at
            if rec[TRACE_OVERFLOW] != 0:
                overflows += 1
                assert term and rows["rewards_sort"][k, j] == rows["rewards_press"][k, j]
                assert rows["rewards_sort"][k, j] == np.float32(rec[TRACE_REWARD] / 2)
            if term:
                o.reset(None)
    assert overflows >= 1
    env.close()


# ---- 4. policy numbers -----------------------------------------------------------------------------------------------
def _w64(policy):
    import torch

    from marl_sortingenv_amd.policy import _shapes

    return {k: torch.tensor(np.asarray(v, dtype=np.float64).reshape(sh))
            for (k, v), sh in zip(policy.weights.items(), _shapes(policy.obs_dim, policy.n_actions))}


@pytest.mark.parametrize("press_masked", [True, False], ids=["masked", "plain"])
def test_fused_modular_rollout_policy_numbers(press_masked):
    """Log-probabilities and values against the float64 restatement of each network on the recorded rows, within the
    bounds the f16x3 form is held to everywhere (LOGP_TOL on the log-probability, LOGIT_TOL on the value); every
    pressing action legal under the mask the agent was shown."""
    import torch

    import marl_sortingenv_amd as M

    n, K = 257, 6
    sort_ag, press_ag = _pair()
    env = _env(n, 0.05, base_seed=3)
    b = M.FusedModularRollout(env, sort_ag, press_ag, K, SORT_SEED, PRESS_SEED, press_masked=press_masked).collect()
    for who, pol, D, A in (("sort", sort_ag, 13, 2), ("press", press_ag, 16, 11)):
        obs = b[f"{who}_obs"].cpu().double().reshape(-1, D)
        mask = (b["press_masks"].cpu().reshape(-1, 11) != 0) if who == "press" and press_masked else None
        _, logsm, value = R.torch_reference(_w64(pol), obs, mask)
        act = b[f"{who}_actions"].cpu().long().reshape(-1)
        assert bool(((act >= 0) & (act < A)).all())
        if mask is not None:
            assert bool(mask.gather(1, act[:, None]).all()), "a masked action was sampled"
        err_p = float((b[f"{who}_log_probs"].cpu().double().reshape(-1) - logsm.gather(1, act[:, None])[:, 0]).abs().max())
        err_v = float((b[f"{who}_values"].cpu().double().reshape(-1) - value).abs().max())
        print(f"{who}: log-probability error {err_p:.3g} (bound {R.LOGP_TOL:g}), value error {err_v:.3g} (bound {R.LOGIT_TOL:g})")
        assert err_p <= R.LOGP_TOL and err_v <= R.LOGIT_TOL
        if mask is None:  # (in an episode of three steps press_action_masks() leaves the presser little choice)
            assert len(torch.unique(act)) == A, f"{who}: the draws do not reach every action"
    env.close()


def _zero_head(D, A, seed):
    import marl_sortingenv_amd as M

    pol = M.MlpPolicy(D, A, R.constant_head_weights(D, A, np.zeros(A, dtype=np.float32), seed=seed), device=0, precision="f16x3")
    assert pol.precision == "f16x3"
    return pol


@pytest.mark.parametrize("press_masked", [True, False], ids=["masked", "plain"])
def test_fused_modular_rollout_sampler_bit_exact_on_zero_heads(press_masked):
    """Zero-head agents (every logit 0): each sampled action equals uniform_sample_f32 of that agent's own word for the
    step, each deterministic one the first legal action; the log-probability is -log(legal count)."""
    import marl_sortingenv_amd as M

    n, K, off = 97, 7, 1000
    env = _env(n, 0.05, base_seed=5, index_offset=off)
    fused = M.FusedModularRollout(env, _zero_head(13, 2, 1), _zero_head(16, 11, 2), K, SORT_SEED, PRESS_SEED,
                                  press_masked=press_masked)
    idx = off + np.arange(n)
    for sdet, pdet in ((False, False), (True, False), (False, True)):
        t0 = env.policy_step
        b = fused.collect(sort_deterministic=sdet, press_deterministic=pdet)
        masks = b["press_masks"].cpu().numpy() != 0
        assert masks.any(axis=2).all()
        for k in range(K):
            shown = masks[k] if press_masked else None
            want_s = np.zeros(n, dtype=np.int64) if sdet else R.uniform_sample_f32(ps.word(SORT_SEED, idx, t0 + k), None, 2)
            if pdet:
                want_p = np.argmax(masks[k], axis=1) if press_masked else np.zeros(n, dtype=np.int64)
            else:
                want_p = R.uniform_sample_f32(ps.word(PRESS_SEED, idx, t0 + k), shown, 11)
            assert np.array_equal(b["sort_actions"][k].cpu().numpy(), want_s), (sdet, pdet, k)
            assert np.array_equal(b["press_actions"][k].cpu().numpy(), want_p), (sdet, pdet, k)
            count = masks[k].sum(axis=1) if press_masked else np.full(n, 11)
            assert np.abs(b["press_log_probs"][k].cpu().numpy() + np.log(count)).max() <= R.LOGP_TOL
            assert np.abs(b["sort_log_probs"][k].cpu().numpy() + np.log(2.0)).max() <= R.LOGP_TOL
    assert env.error_count() == 0
    env.close()


def test_masked_presser_with_several_legal_actions():
    """Beyond the three-step episodes above, in which press_action_masks() rarely offers more than action 0: episodes
    of 40 steps, where the masked pressing agent has a real choice - against the twin, and the zero-head sampler bit for
    bit under those masks."""
    import marl_sortingenv_amd as M

    n, K = 97, 40
    n_done, _ = _compare_with_twin("long episodes", n, 0.05, True, "sampled", (K, 3), max_steps=40)
    assert n_done >= n
    env = _env(n, 0.05, base_seed=5, max_steps=40)
    fused = M.FusedModularRollout(env, _zero_head(13, 2, 1), _zero_head(16, 11, 2), K, SORT_SEED, PRESS_SEED)
    b = fused.collect()
    masks = b["press_masks"].cpu().numpy() != 0
    assert (masks.sum(axis=2) > 1).mean() > 0.05, "the masks leave the presser no choice"
    for k in range(K):
        want = R.uniform_sample_f32(ps.word(PRESS_SEED, np.arange(n), k), masks[k], 11)
        assert np.array_equal(b["press_actions"][k].cpu().numpy(), want), k
    env.close()


# ---- 5. both agents deterministic: the shipped model rollout -----------------------------------------------------------
@pytest.mark.parametrize("noise", [0.0, 0.05], ids=["n0", "n5"])
def test_deterministic_modular_rollout_equals_model_rollout(noise):
    import torch

    import marl_sortingenv_amd as M

    n, K = 257, 7
    sort_ag, press_ag = _pair()
    a, b = _env(n, noise, base_seed=21), _env(n, noise, base_seed=21)
    fused = M.FusedModularRollout(a, sort_ag, press_ag, K + 1, SORT_SEED, PRESS_SEED, press_masked=True)
    for launch in range(2):
        got = fused.collect(K + 1, sort_deterministic=True, press_deterministic=True)
        exp = b.rollout(K + 1, policy="model", sort_agent=sort_ag, press_agent=press_ag, press_agent_maskable=True)
        assert torch.equal(11 * got["sort_actions"] + got["press_actions"], exp["actions"]), launch
        assert torch.equal(got["rewards"].view(torch.int32), exp["reward"].view(torch.int32)), launch
        assert np.array_equal(_dones(got, K + 1), exp["done"].cpu().numpy() != 0), launch
        # the rows the next decision is taken from: both kernels record them before the step
        assert torch.equal(got["sort_obs"].view(torch.int32), exp["sort_obs"].view(torch.int32)), launch
        assert torch.equal(got["press_obs"].view(torch.int32), exp["press_obs"].view(torch.int32)), launch
        # press_action_masks() of step k + 1 = the first 11 entries of the post-step mask of step k
        assert torch.equal(got["press_masks"][1:], exp["mask"][:-1, :, :11]), launch
        _state_equal(f"launch {launch}", a, b)
    a.close()
    b.close()


# ---- 6. memory -------------------------------------------------------------------------------------------------------
def _raw_call(env, sort_ag, press_ag, K, flags, ptrs, sort_seed=SORT_SEED, press_seed=PRESS_SEED, struct_size=None):
    from marl_sortingenv_amd._lib import MODULAR_BUFFER_NAMES, MseModularBuffers

    out = MseModularBuffers(C.sizeof(MseModularBuffers) if struct_size is None else struct_size, 0,
                            *(ptrs.get(name) for name in MODULAR_BUFFER_NAMES))
    return env.L.mse_rollout_modular(env._h, None if sort_ag is None else sort_ag._h,
                                     None if press_ag is None else press_ag._h, K, sort_seed, press_seed, flags,
                                     C.byref(out), None)


def _sizes(n, K):
    return {"sort_obs": K * n * 13 * 4, "press_obs": K * n * 16 * 4, "press_masks": K * n * 11, "episode_starts": K * n,
            "sort_actions": K * n * 4, "press_actions": K * n * 4, "sort_log_probs": K * n * 4, "press_log_probs": K * n * 4,
            "sort_values": K * n * 4, "press_values": K * n * 4, "rewards": K * n * 4, "rewards_sort": K * n * 4,
            "rewards_press": K * n * 4, "sort_last_values": n * 4, "press_last_values": n * 4, "last_dones": n}


def test_fused_modular_rollout_memory():
    import torch

    from marl_sortingenv_amd._lib import MODULAR_BUFFER_NAMES

    n, K = 97, 4
    sort_ag, press_ag = _pair()
    env = _env(n, 0.05, base_seed=9)
    rng_before = env.get_state()[2].clone()
    raw, at = guarded(_sizes(n, K))
    ptrs = {name: raw.data_ptr() + off for name, (off, _) in at.items()}
    assert _raw_call(env, sort_ag, press_ag, K, 64, ptrs) == 0
    torch.cuda.synchronize()
    within = inside(raw, at)
    assert bool((raw[~within] == 0xA5).all()), "a guard byte was written"
    # rng_sorting (words 18-23) and rng_pressing (words 12-17) are not touched: there are no fallback draws
    rng_after = env.get_state()[2]
    assert torch.equal(rng_before[:, 12:24], rng_after[:, 12:24])
    # every output NULL, then one at a time
    assert _raw_call(env, sort_ag, press_ag, K, 64, {}) == 0
    for name in MODULAR_BUFFER_NAMES:
        assert _raw_call(env, sort_ag, press_ag, 1, 64, {name: ptrs[name]}) == 0, name
    torch.cuda.synchronize()
    assert bool((raw[~within] == 0xA5).all())
    assert env.policy_step == K + K + len(MODULAR_BUFFER_NAMES) and env.error_count() == 0
    env.close()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------
# the table image grows with container_capacity (one level per unit): at 8000 it is accepted by mse_create (below the
# 64 KiB of tables a handle may have) and leaves k_rollout_modular's 32-env waves room, but not its 64-env waves
# (142 880 B of images and wave tiles + the tables > 160 KiB)
BIG_TABLES_META = dict(kind="mono", max_steps=MAX_STEPS, noise_sorting=0.05, balesize=200,
                       config_overrides={"pressing_station": {"container_capacity": 8000}})
GEN_META = dict(kind="mono", max_steps=MAX_STEPS, noise_sorting=0.05, balesize=200,
                config_overrides={"simulation": {"input_batch_size": 90}})


def _check_call(env, sort_ag, press_ag, K, flags=0, sort_seed=SORT_SEED, press_seed=PRESS_SEED):
    return env.L.mse_rollout_modular_check(env._h, None if sort_ag is None else sort_ag._h,
                                           None if press_ag is None else press_ag._h, K, sort_seed, press_seed, flags)


def test_fused_modular_rollout_refusals():
    import torch

    import marl_sortingenv_amd as M

    INVALID, UNSUPPORTED, NOT_RESET = -1, -2, -5
    n, K = 64, 2
    sort_ag, press_ag = _pair()
    opened = []

    def keep(e):
        opened.append(e)
        return e

    try:
        env = keep(_env(n, 0.05))
        raw, at = guarded(_sizes(n, K))
        ptrs = {name: raw.data_ptr() + off for name, (off, _) in at.items()}
        assert _check_call(env, sort_ag, press_ag, K) == 0 and env.policy_step == 0  # the check launches nothing
        assert _raw_call(env, sort_ag, press_ag, K, 0, ptrs) == 0
        torch.cuda.synchronize()
        filled, state, t = raw.clone(), [x.clone() for x in env.get_state()], env.policy_step

        def refused(status, e=env, s=sort_ag, p=press_ag, k=K, flags=0, **kw):
            """The check-only entry first: only a call it refuses is sent to the entry that could launch."""
            seeds = {k_: v for k_, v in kw.items() if k_ != "struct_size"}
            if "struct_size" not in kw:
                assert _check_call(e, s, p, k, flags, **seeds) == status
            before = None if e is None or e._h is None else e.policy_step
            assert _raw_call(e, s, p, k, flags, ptrs, **kw) == status
            torch.cuda.synchronize()
            assert torch.equal(raw, filled), "a refused call wrote to the buffers"
            assert before is None or e.policy_step == before

        refused(INVALID, s=None)
        refused(INVALID, p=None)
        refused(INVALID, s=press_ag)
        refused(INVALID, p=sort_ag)
        mono_agent = M.MlpPolicy.random_init(29, 22, seed=3)
        refused(INVALID, s=mono_agent)
        refused(INVALID, p=mono_agent)
        refused(INVALID, sort_seed=7, press_seed=7)
        refused(INVALID, k=0)
        refused(INVALID, k=-1)
        for flag in (1, 4, 8, 16, 32, 512, 1 << 31):  # MSE_STEP_UNMASKED and every bit that is not one of the four
            refused(INVALID, flags=flag)
        refused(INVALID, struct_size=8)
        press_env = keep(M.BatchedSortingEnv(kind="press", num_envs=n, device=0))
        refused(INVALID, e=press_env)
        refused(INVALID, e=keep(M.BatchedSortingEnv(kind="sort", num_envs=n, device=0)))
        no_reset = keep(_env(n, 0.05, auto_reset=False))
        refused(INVALID, e=no_reset)
        refused(NOT_RESET, e=keep(_env(n, 0.05, reset_now=False)))
        env.trace_begin(0, 16)
        refused(INVALID)
        for cls in (M.FusedModularRollout, M.ModularRolloutCollector):
            with pytest.raises(M.MseError) as err:
                cls(env, sort_ag, press_ag, K).collect()
            assert err.value.status == INVALID
        env.trace_end()
        f32_sort = M.MlpPolicy.random_init(13, 2, seed=1, precision="f32")
        refused(UNSUPPORTED, s=f32_sort)
        refused(UNSUPPORTED, p=M.MlpPolicy.random_init(16, 11, seed=2, precision="f32"))
        refused(UNSUPPORTED, e=keep(_env(n, 0.05, literal_choice=True)))
        gen_env = keep(_env(n, 0.05, config=replay.sorting_config(GEN_META)))
        refused(UNSUPPORTED, e=gen_env)
        # tables that do not fit: the same config is served in 32-env waves and refused in 64-env waves
        big_cfg = replay.sorting_config(BIG_TABLES_META)
        small_big = keep(_env(n, 0.05, config=big_cfg))
        assert _check_call(small_big, sort_ag, press_ag, K) == 0
        assert _raw_call(small_big, sort_ag, press_ag, K, 0, ptrs) == 0
        torch.cuda.synchronize()
        filled = raw.clone()
        big = keep(_env(256 * cus() + 1, 0.05, config=big_cfg))
        big_state = [x.clone() for x in big.get_state()]
        refused(UNSUPPORTED, e=big)
        assert b"LDS image does not fit" in big.L.mse_last_error()
        for x, y in zip(big_state, big.get_state()):
            assert torch.equal(x, y)
        assert big.policy_step == 0
        # the env the refusals were tried on is where it was
        for x, y in zip(state, env.get_state()):
            assert torch.equal(x, y)
        assert env.policy_step == t
        # the Python classes refuse the same, both of them
        for cls in (M.FusedModularRollout, M.ModularRolloutCollector):
            with pytest.raises(ValueError):
                cls(env, sort_ag, press_ag, K, sort_seed=5, press_seed=5)
            with pytest.raises(ValueError):
                cls(env, press_ag, sort_ag, K)
            with pytest.raises(ValueError):
                cls(env, sort_ag, None, K)
            with pytest.raises(ValueError):
                cls(no_reset, sort_ag, press_ag, K)
            with pytest.raises(ValueError):
                cls(press_env, sort_ag, press_ag, K)
            with pytest.raises(ValueError):
                cls(env, sort_ag, press_ag, K).collect(K + 1)
            for e, s in ((gen_env, sort_ag), (big, sort_ag), (env, f32_sort)):
                with pytest.raises(M.MseError) as err:
                    cls(e, s, press_ag, K).collect()
                assert err.value.status == UNSUPPORTED
        for x, y in zip(big_state, big.get_state()):
            assert torch.equal(x, y)
        assert big.policy_step == 0 and gen_env.policy_step == 0
        assert M.FusedModularRollout(env, sort_ag, press_ag, K).collect()["rewards"].shape == (K, n)
    finally:
        for e in opened:
            e.close()


def test_twin_reads_episode_starts_off_the_state():
    """The twin carries nothing between calls: built on a handle that has already been stepped, and again after a
    state_dict round trip, its rows - the first episode_starts row among them - are the kernel's."""
    import marl_sortingenv_amd as M

    n, K = 33, 4
    sort_ag, press_ag = _pair()
    a, b, c = (_env(n, 0.05, base_seed=17) for _ in range(3))
    fused = M.FusedModularRollout(a, sort_ag, press_ag, K, SORT_SEED, PRESS_SEED)
    M.FusedModularRollout(b, sort_ag, press_ag, K, SORT_SEED, PRESS_SEED).collect()  # b is one step into its episodes ...
    fused.collect()
    twin = M.ModularRolloutCollector(b, sort_ag, press_ag, K, SORT_SEED, PRESS_SEED)  # ... when the twin first sees it
    got, exp = fused.collect(), twin.collect()
    assert not bool(exp["episode_starts"][0].any()) and bool(exp["episode_starts"][1:].any())
    bits_equal("stepped handle", got, exp, TWIN_KEYS, K)
    sd = twin.state_dict()
    assert sd["collector"] == "modular_twin" and "last_done" not in sd
    other = M.ModularRolloutCollector(c, sort_ag, press_ag, K, SORT_SEED, PRESS_SEED)
    other.load_state_dict(sd)
    bits_equal("restored handle", fused.collect(), other.collect(), TWIN_KEYS, K)
    _state_equal("restored handle", a, c)
    for e in (a, b, c):
        e.close()
