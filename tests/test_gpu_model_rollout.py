"""GPU: Env_3_Monolith.step(action=None, mode='model') at batch scale (env_monolith.py:186-221) - the fused rollout
mse_rollout_model (BatchedSortingEnv.rollout(K, policy="model")) with its sorting / pressing agents evaluated inside
the kernel, against

  * the multi-launch form ModelRolloutCollector (previews, MlpPolicy forwards, mse_model_actions, mse_step): bit for
    bit, every output, the full state with all five PCG64 streams and the policy step counter after every launch;
  * the reference's own mode='model' trajectories without agents (tests/golden/model_mono_*.npz);
  * per-env oracle.OracleEnv replays at the sizes where the launcher switches from 32-env to 64-env waves, the agents'
    argmax restated in float64 torch;
  * and its refusals, one status code each."""
import ctypes as C

import numpy as np
import pytest

from oracle.oracle import OracleEnv
from tests import replay
from tests.rollout_checks import cus
from tests.test_gpu_full_size_oracle import _COL_IDX, _COL_NAME, _check_reward, _same
from tests.test_gpu_golden import SKIP_COLS, _skip_words

pytestmark = pytest.mark.gpu

# sort agent, press agent, press agent maskable
COMBOS = {
    "none": (False, False, True),
    "sort": (True, False, True),
    "press_maskable": (False, True, True),
    "press_plain": (False, True, False),
    "both_maskable": (True, True, True),
    "both_plain": (True, True, False),
}
KEYS = ("actions", "obs", "reward", "done", "mask", "sort_obs", "press_obs")


def _env(n, noise, max_steps, base_seed=0, **kw):
    import marl_sortingenv_amd as M

    kw.setdefault("auto_reset", True)
    return M.BatchedSortingEnv(kind="mono", num_envs=n, device=0, base_seed=base_seed, max_steps=max_steps,
                               noise_sorting=noise, balesize=200, **kw)


def _agents(combo, seed=0, head_gain=1.0):
    """MlpPolicy.random_init agents in the f16x3 form; head_gain scales the action head (SB3's initial 0.01 leaves the
    logits of a fresh network within ~1e-2 of each other)."""
    import marl_sortingenv_amd as M

    use_sort, use_press, maskable = COMBOS[combo]
    out = []
    for use, d, a, s in ((use_sort, 13, 2, seed + 1), (use_press, 16, 11, seed + 2)):
        if not use:
            out.append(None)
            continue
        p = M.MlpPolicy.random_init(d, a, seed=s, precision="f16x3")
        if head_gain != 1.0:
            w = dict(p.weights)
            w["action_net.weight"] = w["action_net.weight"] * np.float32(head_gain)
            p = M.MlpPolicy(d, a, {k: v.reshape(sh) for (k, v), sh in zip(w.items(), _shapes(d, a))}, precision="f16x3")
        assert p.precision == "f16x3"
        out.append(p)
    return out[0], out[1], maskable


def _shapes(d, a):
    from marl_sortingenv_amd.policy import _shapes as shapes

    return shapes(d, a)


def _state_equal(tag, a, b):
    import torch

    for name, x, y in zip(("ints", "dbls", "rng"), a.get_state(), b.get_state()):
        if not torch.equal(x, y):
            bad = torch.nonzero((x != y).reshape(x.shape[0], -1).any(dim=1)).flatten()
            raise AssertionError(f"{tag}: {name} of {bad.numel()} envs differ, first env {int(bad[0])}")
    assert a.policy_step == b.policy_step, tag


# ---- 1. fused == multi-launch, bit for bit ---------------------------------------------------------------------------
@pytest.mark.parametrize("noise", [0.0, 0.05], ids=["n0", "n5"])
@pytest.mark.parametrize("masking", [True, False], ids=["masked", "unmasked"])
@pytest.mark.parametrize("combo", list(COMBOS))
def test_fused_model_rollout_matches_multi_launch(combo, masking, noise):
    import torch

    import marl_sortingenv_amd as M

    sort_ag, press_ag, maskable = _agents(combo)
    for n in (300, 4097):  # 4097: a ragged last wave
        fused, multi = _env(n, noise, 30, base_seed=11), _env(n, noise, 30, base_seed=11)
        coll = M.ModelRolloutCollector(multi, sort_agent=sort_ag, press_agent=press_ag, press_agent_maskable=maskable)
        n_done = 0
        for K in (64, 1, 17):  # max_steps 30: auto-resets inside and across launches
            tag = f"{combo} masking={masking} noise={noise} n={n} K={K}"
            got = fused.rollout(K, policy="model", sort_agent=sort_ag, press_agent=press_ag,
                                press_agent_maskable=maskable, use_action_masking=masking)
            exp = coll.collect(K, use_action_masking=masking)
            for key in KEYS:
                x, y = got[key], exp[key]
                if x.dtype == torch.float32:
                    x, y = x.view(torch.int32), y.view(torch.int32)
                if not torch.equal(x, y):
                    bad = torch.nonzero((x != y).reshape(K, n, -1).any(dim=2))
                    raise AssertionError(f"{tag}: {key} differs at {bad.shape[0]} (step, env) rows, first {bad[0].tolist()}")
            _state_equal(tag, fused, multi)
            n_done += int(exp["done"].sum())
        assert n_done >= 2 * n  # every episode ended twice inside the first launch
        fused.close()
        multi.close()


# ---- 2. the reference's trajectories, no agents ----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["model_mono_n0_masked_s2_s17", "model_mono_n5_unmasked_s4_s23"])
def test_fused_model_rollout_matches_reference_fixture(name):
    import torch

    path = replay.GOLDEN_DIR + "/" + name + ".npz"
    meta, z = replay.load(path)
    starts = np.flatnonzero(z["op"] == 1)
    seeds = [int(z["arg"][r]) for r in starts]
    env = _env(len(seeds), meta["noise_sorting"], 200, seeds=torch.tensor(seeds, dtype=torch.int64))
    masking = bool(meta["masking"])
    first = env.rollout(198, policy="model", use_action_masking=masking)
    acc_before = env.get_state()[1].cpu().numpy()  # accuracy_sorter of step 199 = accuracy_belt after step 198
    last = env.rollout(1, policy="model", use_action_masking=masking)
    rows = {k: torch.cat([first[k], last[k]]).cpu().numpy() for k in ("actions", "obs", "reward", "done", "mask")}
    ints, dbls, rng = (x.cpu().numpy() for x in env.get_state())
    rng = rng.view(np.uint64)
    for j, r0 in enumerate(starts):
        for t in range(1, 200):
            row, tag = r0 + t, f"{name} seed {seeds[j]} step {t}"
            assert rows["actions"][t - 1, j] == int(z["arg"][row]), tag
            _same(f"{tag}: obs", rows["obs"][t - 1, j][None], z["obs"][row][None])
            assert np.array_equal(rows["mask"][t - 1, j], z["mask"][row]), tag
            assert int(rows["done"][t - 1, j]) == int(z["terminated"][row]), tag
            _check_reward(tag, rows["reward"][t - 1, j:j + 1], z["reward"][row:row + 1])
        snap = (ints[j], np.concatenate([dbls[j], acc_before[j]]), rng[j])
        replay.compare_row(name, z, r0 + 199, rows["obs"][198, j], float(z["reward"][r0 + 199]), False,
                           rows["mask"][198, j], snap, 1e-6, SKIP_COLS, _skip_words(meta))
    env.close()


# ---- 3. the oracle at the sizes of both launch shapes ----------------------------------------------------------------
def _actor64(policy):
    """The agent's actor in float64 torch: tanh MLP, linear head."""
    import torch

    w = {k: torch.tensor(v, dtype=torch.float64) for k, v in policy.weights.items()}
    H = 32

    def f(x):
        x = torch.as_tensor(x, dtype=torch.float64)
        h = torch.tanh(x @ w["mlp_extractor.policy_net.0.weight"].reshape(H, -1).T + w["mlp_extractor.policy_net.0.bias"])
        h = torch.tanh(h @ w["mlp_extractor.policy_net.2.weight"].reshape(H, H).T + w["mlp_extractor.policy_net.2.bias"])
        return h @ w["action_net.weight"].reshape(policy.n_actions, H).T + w["action_net.bias"]

    return f


def _check_argmax(tag, got, logits, mask=None):
    """got[r] must be the first argmax of logits[r] (masked to -1e8), or an action whose float64 logit is within 1e-4
    of the maximum (the f16x3 products decide near-ties; an all-zero observation at an episode's start ties every
    action of a bias-free network exactly)."""
    import torch

    lg = logits.clone()
    if mask is not None:
        lg[~mask] = -1e8
    first = lg.argmax(dim=-1).numpy()  # torch.argmax returns the first maximum
    top = lg.max(dim=-1).values
    near = (lg.gather(1, torch.as_tensor(got, dtype=torch.int64)[:, None])[:, 0] >= top - 1e-4).numpy()
    ok = (got == first) | near
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, f"{tag}: agent action {int(got[bad[0]])} vs argmax {int(first[bad[0]])} at row {int(bad[0])}"


def _replay_oracle(tag, rows, envs, orcs, sort_ag, press_ag, press_masked, masking):
    """rows: the rollout's [K, S, ...] rows of the sampled envs; orcs: their OracleEnvs in the state the rollout
    started from.  Previews, agent parts, drawn parts and every transition."""
    import torch

    K = rows["actions"].shape[0]
    sort_f = None if sort_ag is None else _actor64(sort_ag)
    press_f = None if press_ag is None else _actor64(press_ag)
    press_masks = np.zeros((K, len(envs), 11), dtype=bool)
    for k in range(K):
        for j, o in enumerate(orcs):
            at = f"{tag}: step {k} env {envs[j]}"
            _same(f"{at}: sort_obs", rows["sort_obs"][k, j][None], o.sort_agent_obs()[None])
            _same(f"{at}: press_obs", rows["press_obs"][k, j][None], o.press_agent_obs()[None])
            press_masks[k, j] = o.action_masks()[:11] != 0
            a = int(rows["actions"][k, j])
            drawn = o.model_action(masking, draw_sort=sort_ag is None, draw_press=press_ag is None)
            if sort_ag is None:
                assert a // 11 == drawn // 11, f"{at}: sorting draw {a // 11} vs {drawn // 11}"
            if press_ag is None:
                assert a % 11 == drawn % 11, f"{at}: press draw {a % 11} vs {drawn % 11}"
            obs, r64, term = o.step(a, check_overflow=False)
            if term:
                obs = o.reset(None)
            _same(f"{at}: obs", rows["obs"][k, j][None], obs[None])
            _same(f"{at}: mask", rows["mask"][k, j][None], o.action_masks()[None])
            assert int(rows["done"][k, j]) == int(term), at
            _check_reward(at, rows["reward"][k, j:j + 1], np.array([r64]))
    acts = rows["actions"].reshape(-1)
    if sort_f is not None:
        _check_argmax(f"{tag}: sorting agent", acts // 11, sort_f(rows["sort_obs"].reshape(-1, 13)))
    if press_f is not None:
        _check_argmax(f"{tag}: pressing agent", acts % 11, press_f(rows["press_obs"].reshape(-1, 16)),
                      torch.as_tensor(press_masks.reshape(-1, 11)) if press_masked else None)


def _final_state(tag, env, envs, orcs, noise, gen=False):
    ints, dbls, rng = (x.cpu().numpy() for x in env.get_state())
    rng = rng.view(np.uint64)
    words = list(range(0, 4)) + list(range(12, 24)) + (list(range(6, 10)) if noise else []) + \
            (list(range(24, 30)) if gen else [])
    for j, o in enumerate(orcs):
        I, D, R = o.snapshot()
        i = envs[j]
        neq = ints[i, _COL_IDX] != I[_COL_IDX]
        assert not neq.any(), f"{tag}: env {i} state differs in {sorted({_COL_NAME[c] for c in np.flatnonzero(neq)})}"
        _same(f"{tag}: env {i} accuracies", dbls[i][None], D[:4][None])
        _same(f"{tag}: env {i} PCG64 words", rng[i, words][None], R[words][None])


@pytest.mark.parametrize("run", ["both_maskable_n5", "sort_unmasked_n0"])
@pytest.mark.parametrize("per_cu", [256, 512], ids=["k_rollout_model_tiles1", "k_rollout_model_tiles2"])
def test_fused_model_rollout_matches_oracle_at_size(per_cu, run):
    import torch

    n, base = per_cu * cus(), 5000
    combo, noise, masking = ("both_maskable", 0.05, True) if run == "both_maskable_n5" else ("sort", 0.0, False)
    sort_ag, press_ag, maskable = _agents(combo, seed=7, head_gain=20.0)
    env = _env(n, noise, 25, base_seed=base)
    # ~512 envs: the first and the last wave, then every 128th (every 256th at the larger size)
    envs = np.unique(np.concatenate([np.arange(64), np.arange(n - 64, n), np.arange(0, n, max(128, n // 512))]))
    orcs = [OracleEnv(kind="mono", max_steps=25, seed=base + int(i), noise_sorting=noise) for i in envs]
    for o, i in zip(orcs, envs):
        o.reset(base + int(i))
    buf = env.rollout(40, policy="model", sort_agent=sort_ag, press_agent=press_ag, press_agent_maskable=maskable,
                      use_action_masking=masking)
    idx = torch.as_tensor(envs, device=env.device)
    rows = {k: buf[k].index_select(1, idx).cpu().numpy() for k in KEYS}
    tag = f"n={n} {run}"
    _replay_oracle(tag, rows, envs, orcs, sort_ag, press_ag, press_ag is not None and masking and maskable, masking)
    _final_state(tag, env, envs, orcs, noise)
    assert rows["done"].sum() > 0
    env.close()


# ---- 4. refusals, and the multi-launch form on a handle the kernel refuses --------------------------------------------
def _rc(env, sort_ag=None, press_ag=None, flags=0, bufs=None, K=2):
    bufs = bufs or {}

    def p(key):
        v = bufs.get(key)
        return None if v is None else C.c_void_p(v)

    return env.L.mse_rollout_model(env._h, None if sort_ag is None else sort_ag._h,
                                   None if press_ag is None else press_ag._h, K, flags, p("actions"), p("obs"),
                                   p("reward"), p("done"), p("mask"), p("sort_obs"), p("press_obs"), None)


def test_fused_model_rollout_refusals():
    import torch

    import marl_sortingenv_amd as M

    INVALID, UNSUPPORTED, NOT_RESET, ALIGNMENT = -1, -2, -5, -6
    env = _env(64, 0.05, 30)
    sort_ag, press_ag, _ = _agents("both_maskable")
    assert _rc(env, sort_ag, press_ag) == 0
    press_env = M.BatchedSortingEnv(kind="press", num_envs=64, device=0)
    assert _rc(press_env) == INVALID
    assert _rc(env, sort_ag=press_ag) == INVALID and _rc(env, press_ag=sort_ag) == INVALID
    mono_agent = M.MlpPolicy.random_init(29, 22, seed=3)
    assert _rc(env, sort_ag=mono_agent) == INVALID and _rc(env, press_ag=mono_agent) == INVALID
    if torch.cuda.device_count() > 1:
        other = M.MlpPolicy.random_init(13, 2, seed=1, device=1)
        assert _rc(env, sort_ag=other) == INVALID
    assert _rc(env, flags=128) == INVALID and _rc(env, flags=8) == INVALID
    env.trace_begin(0, 16)
    assert _rc(env) == INVALID
    env.trace_end()
    assert _rc(_env(64, 0.05, 30, auto_reset=False)) == INVALID
    assert _rc(_env(64, 0.05, 30, reset_now=False)) == NOT_RESET
    assert _rc(env, K=0) == INVALID
    raw = torch.empty(4 * 64 * 64 + 16, dtype=torch.uint8, device=env.device)
    for key in ("obs", "mask", "sort_obs", "press_obs"):
        assert _rc(env, bufs={key: raw.data_ptr() + 4}, K=1) == ALIGNMENT, key
    f32_agent = M.MlpPolicy.random_init(16, 11, seed=2, precision="f32")
    assert _rc(env, press_ag=f32_agent) == UNSUPPORTED
    assert _rc(_env(64, 0.05, 30, literal_choice=True)) == UNSUPPORTED
    gen_meta = dict(kind="mono", max_steps=30, noise_sorting=0.05, balesize=200,
                    config_overrides={"simulation": {"input_batch_size": 90}})
    gen_env = _env(64, 0.05, 30, config=replay.sorting_config(gen_meta))
    assert _rc(gen_env) == UNSUPPORTED
    with pytest.raises(M.MseError) as e:
        gen_env.rollout(4, policy="model")
    assert e.value.status == UNSUPPORTED and "ModelRolloutCollector" in str(e.value)
    with pytest.raises(ValueError):
        env.rollout(4, policy="modle")
    assert env.rollout(3, policy="random")["actions"].shape == (3, 64)  # the other policies are untouched
    assert env.rollout(3, policy="rule_based")["actions"].shape == (3, 64)


def test_model_collector_in_general_generator_mode_matches_oracle():
    """input_batch_size 90: the generator's remainder draws run on the device, which the fused kernel does not serve;
    ModelRolloutCollector does, and matches per-env OracleEnv."""
    import marl_sortingenv_amd as M

    n, base, noise = 64, 300, 0.05
    meta = dict(kind="mono", max_steps=20, noise_sorting=noise, balesize=200,
                config_overrides={"simulation": {"input_batch_size": 90}})
    env = _env(n, noise, 20, base_seed=base, config=replay.sorting_config(meta))
    orcs = [OracleEnv(kind="mono", seed=base + i, cfg=replay.oracle_config(meta)) for i in range(n)]
    for i, o in enumerate(orcs):
        o.reset(base + i)
    sort_ag, press_ag, _ = _agents("both_maskable", seed=4, head_gain=20.0)
    for launch, (s, p, masking) in enumerate(((sort_ag, press_ag, True), (None, None, True), (None, press_ag, False))):
        coll = M.ModelRolloutCollector(env, sort_agent=s, press_agent=p)
        buf = coll.collect(25, use_action_masking=masking)
        rows = {k: buf[k].cpu().numpy() for k in KEYS}
        _replay_oracle(f"generator mode, launch {launch}", rows, np.arange(n), orcs, s, p, p is not None and masking,
                       masking)
    _final_state("generator mode", env, np.arange(n), orcs, noise, gen=True)
    env.close()
