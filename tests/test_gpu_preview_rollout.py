"""GPU: the preview rollout (mse_rollout_policy_preview; FusedPolicyRollout(view="preview")) - K steps of Env_3 in one
launch with one 29 -> 22 network acting on the observation AFTER the step's flow update, the rule-based controller's label
and DAgger's who-steps mixture in the same launch - against

  * its multi-launch twin PolicyRolloutCollector(view="preview") and a hand loop of the sentence in include/mse.h
    (mse_mono_agent_obs, mse_action_masks, mse_rule_actions, mse_policy_forward, mse_demo_who_steps_host, mse_step): every
    buffer, the mse_get_state record and the step counter, on bits, at every shape the plan gives;
  * per-env oracle.OracleEnv replays of the recorded stepped actions, and the float64 network of
    tests/policy_head_reference.py on the recorded rows;
  * contracts (b) and (c) of the header, guard bytes, NULL outputs, and every refusal in the header's order.

max_steps = 7 with K = 17 crosses the auto-reset twice inside one launch."""
import ctypes as C

import numpy as np
import pytest

from oracle.oracle import OracleEnv
from tests import policy_head_reference as R
from tests.rollout_checks import bits_equal, cus, guarded, inside, overflow_config, who_host
from tests.test_demo_mixture_cpu import who_steps
from tests.test_gpu_demo_rollout import BIG_TABLES, GEN, _actor
from tests.test_gpu_full_size_oracle import _check_reward, _same
from tests.test_gpu_model_rollout import _final_state, _state_equal
from tests.test_gpu_modular_rollout import _w64

pytestmark = pytest.mark.gpu

SEED, MIX_SEED, ONE = 77, 99, 1 << 24
MAX_STEPS, K17 = 7, 17
CHECK_OVERFLOW, DETERMINISTIC = 2, 1024  # MSE_STEP_CHECK_OVERFLOW, MSE_PREVIEW_DETERMINISTIC
KEYS = ("observations", "action_masks", "episode_starts", "actions", "log_probs", "values", "rewards", "expert_actions",
        "stepped_actions", "expert_stepped", "last_values", "last_dones")  # struct mse_preview_buffers, in its order
LABEL_KEYS = ("expert_actions", "stepped_actions", "expert_stepped")
COLLECTOR_KEYS = ("observations", "action_masks", "actions", "log_probs", "values", "rewards", "episode_starts", "expert_actions",
                  "last_values", "last_dones")
SNAP_CURRENT_STEP = 32  # column of mse_get_state's integer record that holds the env's current_step


def _env(n, noise=0.05, max_steps=MAX_STEPS, base_seed=11, **kw):
    import marl_sortingenv_amd as M

    kw.setdefault("auto_reset", True)
    return M.BatchedSortingEnv(kind="mono", num_envs=n, device=0, base_seed=base_seed, max_steps=max_steps,
                               noise_sorting=noise, balesize=200, **kw)


def _buffers(n, K, names=KEYS):
    import torch

    from marl_sortingenv_amd.collector import ROW_DTYPES

    shapes = {"observations": (K, n, 29), "action_masks": (K, n, 22), "last_values": (n,), "last_dones": (n,)}
    return {k: torch.zeros(shapes.get(k, (K, n)), dtype=ROW_DTYPES[k], device="cuda:0") for k in names}


def _launch(env, pol, K, ptrs, threshold=0, flags=0, seed=SEED, mix_seed=MIX_SEED, struct_size=None, no_out=False):
    """mse_rollout_policy_preview with `ptrs` {member: address}; members left out are NULL.  -> the status."""
    from marl_sortingenv_amd._lib import PREVIEW_BUFFER_NAMES, MsePreviewBuffers

    out = MsePreviewBuffers(C.sizeof(MsePreviewBuffers) if struct_size is None else struct_size, 0,
                            *(ptrs.get(name) for name in PREVIEW_BUFFER_NAMES))
    return env.L.mse_rollout_policy_preview(None if env is None else env._h, None if pol is None else pol._h, K, seed, mix_seed,
                                            threshold, flags, None if no_out else C.byref(out), None)


def _check_call(env, pol, K, threshold=0, flags=0, seed=SEED, mix_seed=MIX_SEED):
    return env.L.mse_rollout_policy_preview_check(None if env is None else env._h, None if pol is None else pol._h, K, seed,
                                                  mix_seed, threshold, flags)


def fused(env, pol, K, threshold=0, flags=0, names=KEYS):
    import torch

    b = _buffers(env.num_envs, K, names)
    assert _launch(env, pol, K, {k: v.data_ptr() for k, v in b.items()}, threshold, flags) == 0, env.L.mse_last_error()
    torch.cuda.synchronize()
    return b


def hand_collect(env, pol, K, threshold=0, deterministic=False, check_overflow=False):
    """The header's sentence: K rounds of mse_mono_agent_obs, the mask read, mse_rule_actions, mse_policy_forward (SEED, t =
    the handle's counter, index_offset = the env's), the host who-steps rule, mse_step; then the critic on the preview of the
    final state."""
    import torch

    b = _buffers(env.num_envs, K)
    last_done = (env.get_state()[0][:, SNAP_CURRENT_STEP] == 0).to(torch.uint8)
    for k in range(K):
        t = env.policy_step
        obs, mask = env.mono_agent_obs(), env.action_masks()
        rule = env.rule_actions()
        out = pol.forward(obs, mask, seed=SEED, t=t, deterministic=deterministic, index_offset=env.index_offset)
        who = torch.from_numpy(who_host(env, MIX_SEED, t, threshold)).to(env.device)
        stepped = torch.where(who != 0, rule, out["action"])
        for key, v in (("observations", obs), ("action_masks", mask), ("episode_starts", last_done), ("actions", out["action"]),
                       ("log_probs", out["logp"]), ("values", out["value"]), ("expert_actions", rule), ("stepped_actions", stepped),
                       ("expert_stepped", who)):
            b[key][k].copy_(v)
        _, rew, done, _ = env.step(stepped, check_overflow=check_overflow)
        b["rewards"][k].copy_(rew)
        last_done = done.clone()
    b["last_values"].copy_(pol.forward(env.mono_agent_obs(), env.action_masks(), seed=SEED, t=env.policy_step, deterministic=True,
                                       index_offset=env.index_offset)["value"])
    b["last_dones"].copy_(last_done)
    return b


def _n_done(b):
    return int(b["episode_starts"][1:].sum()) + int(b["last_dones"].sum())


# ---- 1. fused == twin == hand loop -------------------------------------------------------------------------------------------
def _compare_all(tag, n, noise, K, precision="f16x3", deterministic=False, **kw):
    """Four handles from one seed: the fused collector, its twin, the raw launch with every member of the struct, the hand
    loop.  Every buffer, the state record and the counter."""
    import marl_sortingenv_amd as M

    pol = _actor("mono", precision)
    a, b, c, d = (_env(n, noise, **kw) for _ in range(4))
    col = M.FusedPolicyRollout(a, pol, K, seed=SEED, view="preview", expert_labels=True)
    twin = M.PolicyRolloutCollector(b, pol, K, seed=SEED, view="preview", expert_labels=True)
    got, exp = col.collect(deterministic=deterministic), twin.collect(deterministic=deterministic)
    bits_equal(f"{tag} twin", got, exp, COLLECTOR_KEYS)
    raw = fused(c, pol, K, 0, DETERMINISTIC if deterministic else 0)
    hand = hand_collect(d, pol, K, 0, deterministic)
    bits_equal(f"{tag} hand", raw, hand, KEYS)
    bits_equal(f"{tag} collector vs raw", got, raw, COLLECTOR_KEYS)
    for other, name in ((b, "twin"), (c, "raw"), (d, "hand")):
        _state_equal(f"{tag} {name}", a, other)
    assert a.policy_step == K and a.error_count() == 0
    assert not bool(raw["expert_stepped"].any()) and bool((raw["stepped_actions"] == raw["actions"]).all())
    mask = raw["action_masks"].cpu().numpy() != 0
    act = raw["actions"].cpu().numpy()
    assert np.take_along_axis(mask, act[..., None], axis=2).all(), "a masked action was drawn"
    n_done = _n_done(raw)
    for e in (a, b, c, d):
        e.close()
    return n_done, raw


@pytest.mark.parametrize("noise", [0.0, 0.05], ids=["n0", "n5"])
@pytest.mark.parametrize("n", [1, 33, 257])
def test_preview_rollout_matches_twin_and_hand_loop(n, noise):
    """A lone lane with mirrors, a second 32-env wave holding one env, a second workgroup holding one env; 17 steps of
    7-step episodes: the auto-reset is crossed twice."""
    n_done, raw = _compare_all(f"n={n} noise={noise}", n, noise, K17)
    assert n_done == 2 * n
    if n > 1:
        assert bool((raw["actions"] != raw["expert_actions"]).any()), "an untrained policy does not act like the expert"


@pytest.mark.parametrize("noise", [0.0, 0.05], ids=["n0", "n5"])
def test_preview_rollout_in_64_env_waves(noise):
    """256 x CUs + 1 envs: the smallest batch plan_policy_plain gives two tiles per wave in the f16x3 form."""
    _compare_all("tiles=2", 256 * cus() + 1, noise, 3)


@pytest.mark.parametrize("noise", [0.0, 0.05], ids=["n0", "n5"])
def test_preview_rollout_exact_f32(noise):
    """The exact-f32 form: 64-env waves, four per workgroup; 65 envs put one env into a second wave."""
    n_done, _ = _compare_all("f32", 65, noise, K17, precision="f32")
    assert n_done == 2 * 65


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_preview_rollout_deterministic(precision):
    _, raw = _compare_all(f"argmax {precision}", 257, 0.05, K17, precision=precision, deterministic=True)
    # the argmax of the float64 network wherever its lead is clear
    import torch

    obs = raw["observations"].cpu().double().reshape(-1, 29)
    mask = raw["action_masks"].cpu().reshape(-1, 22) != 0
    logits, _, _ = R.torch_reference(_w64(_actor("mono", precision)), obs, mask)
    top2 = torch.topk(logits, 2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > 10 * R.LOGIT_TOL
    act = raw["actions"].cpu().long().reshape(-1)
    assert bool(clear.any()) and bool((act[clear] == logits.argmax(dim=1)[clear]).all())


# ---- 2. the mixture, and check_overflow --------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("n", [33, 257])
def test_preview_mixture_matches_the_hand_loop(n, beta):
    import torch

    import marl_sortingenv_amd as M

    pol, threshold = _actor("mono"), M.expert_threshold(beta)
    a, b = _env(n), _env(n)
    t = 0
    for K in (5, 1, K17):
        got, exp = fused(a, pol, K, threshold), hand_collect(b, pol, K, threshold)
        bits_equal(f"n={n} beta={beta} K={K}", got, exp, KEYS)
        _state_equal(f"n={n} beta={beta} K={K}", a, b)
        who = got["expert_stepped"].cpu().numpy()
        for k in range(K):  # the library's host rule, and the numpy restatement of it
            assert np.array_equal(who[k], who_host(a, MIX_SEED, t + k, threshold)), (K, k)
            assert np.array_equal(who[k], who_steps(n, 0, MIX_SEED, t + k, threshold)), (K, k)
        es = got["expert_stepped"] != 0
        assert torch.equal(got["stepped_actions"], torch.where(es, got["expert_actions"], got["actions"]))
        if K == K17:
            share = float(who.mean())
            assert share == beta if beta in (0.0, 1.0) else 0.35 < share < 0.65
            assert bool((got["actions"] != got["expert_actions"]).any())  # the policy's own draw is kept whoever steps
        t += K
    assert a.policy_step == t == 23
    a.close()
    b.close()


def test_preview_mixture_on_a_shard():
    """index_offset enters both stream keys: 33 envs at offset 224 are rows 224..256 of the 257-env run."""
    import torch

    pol = _actor("mono")
    whole, shard = _env(257), _env(33, index_offset=224)  # env j of the shard is seeded base_seed + 224 + j
    w, s = fused(whole, pol, K17, 1 << 23), fused(shard, pol, K17, 1 << 23)
    for key in KEYS:
        x = w[key][224:] if w[key].dim() == 1 else w[key][:, 224:]
        assert torch.equal(x.contiguous().view(torch.uint8), s[key].contiguous().view(torch.uint8)), key
    whole.close()
    shard.close()


@pytest.mark.parametrize("noise", [0.0, 0.05], ids=["n0", "n5"])
def test_preview_rollout_check_overflow(noise):
    """check_overflow at container capacity 30: episodes end by overflow with the termination penalty as the reward."""
    from marl_sortingenv_amd.config import SortingEnvConfig

    pen = np.float32(SortingEnvConfig().overflow_termination_penalty)
    pol, n = _actor("mono"), 257
    cfg = overflow_config(noise)
    a, b = _env(n, noise, config=cfg), _env(n, noise, config=cfg)
    got = fused(a, pol, K17, 1 << 23, CHECK_OVERFLOW)
    exp = hand_collect(b, pol, K17, 1 << 23, check_overflow=True)
    bits_equal(f"overflow noise={noise}", got, exp, KEYS)
    _state_equal(f"overflow noise={noise}", a, b)
    assert int((got["rewards"] == float(pen)).sum()) >= 1, "no episode ended by overflow"
    a.close()
    b.close()


# ---- 3. the oracle -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_preview_rollout_matches_oracle(precision):
    """N = 300, K = 20, nine-step episodes, the mixture at one half: the first and last lane of the first wave, the first
    lane of the second, the last and first env of a workgroup boundary (32-env waves; in the f32 form lanes of 64-env
    waves), the last env - replayed through OracleEnv with the recorded stepped actions."""
    import torch

    n, K, max_steps, base, noise = 300, 20, 9, 500, 0.05
    pol = _actor("mono", precision)
    env = _env(n, noise, max_steps=max_steps, base_seed=base)
    envs = [0, 31, 32, 255, 256, 299]
    orcs = [OracleEnv(kind="mono", max_steps=max_steps, seed=base + i, noise_sorting=noise) for i in envs]
    for o, i in zip(orcs, envs):
        o.reset(base + i)
    b = fused(env, pol, K, 1 << 23)
    rows = {k: v.cpu().numpy() for k, v in b.items()}
    dones = np.concatenate([rows["episode_starts"][1:], rows["last_dones"][None]]) != 0
    for k in range(K):
        for o, i in zip(orcs, envs):
            at = f"step {k} env {i}"
            view = np.concatenate([o.sort_agent_obs(), o.press_agent_obs()])
            _same(f"{at}: observations", rows["observations"][k, i][None], view[None])
            _same(f"{at}: action_masks", rows["action_masks"][k, i][None], o.action_masks().astype(np.uint8)[None])
            _, r64, term = o.step(int(rows["stepped_actions"][k, i]), check_overflow=False)
            _check_reward(at, rows["rewards"][k, i:i + 1], np.array([r64]))
            assert bool(dones[k, i]) == bool(term), at
            if term:
                o.reset(None)
    assert dones[:, envs].sum() >= 2 * len(envs)
    _final_state("oracle", env, envs, orcs, noise)
    # the network's numbers on every recorded row, against the float64 restatement
    obs = b["observations"].cpu().double().reshape(-1, 29)
    mask = b["action_masks"].cpu().reshape(-1, 22) != 0
    _, logsm, value = R.torch_reference(_w64(pol), obs, mask)
    act = b["actions"].cpu().long().reshape(-1)
    assert bool(mask.gather(1, act[:, None]).all()), "a masked action was sampled"
    err_p = float((b["log_probs"].cpu().double().reshape(-1) - logsm.gather(1, act[:, None])[:, 0]).abs().max())
    err_v = float((b["values"].cpu().double().reshape(-1) - value).abs().max())
    print(f"{precision}: log-probability error {err_p:.3g} (bound {R.LOGP_TOL:g}), value error {err_v:.3g} (bound {R.LOGIT_TOL:g})")
    assert err_p <= R.LOGP_TOL and err_v <= R.LOGIT_TOL
    last = torch.from_numpy(np.stack([np.concatenate([o.sort_agent_obs(), o.press_agent_obs()]) for o in orcs])).double()
    _, _, v_end = R.torch_reference(_w64(pol), last, torch.ones((len(envs), 22), dtype=torch.bool))
    assert float((b["last_values"].cpu().double()[envs] - v_end).abs().max()) <= R.LOGIT_TOL
    env.close()


# ---- 4. contracts (b) and (c) ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [33, 257])
def test_contract_b_label_pointers_change_nothing_at_threshold_0(n):
    pol = _actor("mono")
    a, b = _env(n), _env(n)
    plain_keys = tuple(k for k in KEYS if k not in LABEL_KEYS)
    for K in (5, K17):
        with_labels, without = fused(a, pol, K), fused(b, pol, K, names=plain_keys)
        bits_equal(f"n={n} K={K}", with_labels, without, plain_keys)
        _state_equal(f"n={n} K={K}", a, b)
    assert a.policy_step == b.policy_step == 22
    a.close()
    b.close()


@pytest.mark.parametrize("noise", [0.0, 0.05], ids=["n0", "n5"])
def test_contract_c_threshold_one_is_the_rule_based_rollout(noise):
    import torch

    pol, n = _actor("mono"), 257
    a, b = _env(n, noise), _env(n, noise)
    for K in (5, K17):
        got = fused(a, pol, K, ONE)
        exp = b.rollout(K, policy="rule_based")
        assert torch.equal(got["stepped_actions"], exp["actions"][:K]) and torch.equal(got["expert_actions"], exp["actions"][:K])
        assert torch.equal(got["rewards"].view(torch.int32), exp["reward"][:K].view(torch.int32))
        assert bool(got["expert_stepped"].all())
        for x, y in zip(a.get_state(), b.get_state()):
            assert torch.equal(x, y)
    a.close()
    b.close()


# ---- 5. memory -----------------------------------------------------------------------------------------------------------------
def _sizes(n, K):
    sizes = {"observations": K * n * 29 * 4, "action_masks": K * n * 22, "episode_starts": K * n, "actions": K * n * 4,
             "log_probs": K * n * 4, "values": K * n * 4, "rewards": K * n * 4, "expert_actions": K * n * 4,
             "stepped_actions": K * n * 4, "expert_stepped": K * n, "last_values": n * 4, "last_dones": n}
    assert tuple(sizes) == KEYS
    return sizes


@pytest.mark.parametrize("n", [97, 65])
def test_preview_rollout_memory(n):
    """n = 97: 32-env waves with a ragged last one; n = 65 with the f32 policy: 64-env waves, one env in the second."""
    import torch

    K = 4
    pol = _actor("mono", "f16x3" if n == 97 else "f32")
    env = _env(n, base_seed=9, max_steps=3)
    rng_before = env.get_state()[2].clone()
    raw, at = guarded(_sizes(n, K))
    ptrs = {name: raw.data_ptr() + off for name, (off, _) in at.items()}
    per_env = ("last_values", "last_dones")
    # K - 1 steps into buffers of K rows: the last row of every [K, N, ...] buffer stays untouched, like the guards
    assert _launch(env, pol, K - 1, ptrs, 1 << 23) == 0
    torch.cuda.synchronize()
    short = inside(raw, at, lambda name, size: size if name in per_env else size // K * (K - 1))
    assert bool((raw[~short] == 0xA5).all()), "a byte past the first K - 1 rows was written"
    assert _launch(env, pol, K, ptrs, 1 << 23) == 0
    torch.cuda.synchronize()
    within = inside(raw, at)
    assert bool((raw[~within] == 0xA5).all()), "a guard byte was written"
    # rng_pressing (words 12-17) and rng_sorting (words 18-23) are neither read nor written, whoever steps
    assert torch.equal(rng_before[:, 12:24], env.get_state()[2][:, 12:24])
    # every output NULL, then each output NULL in turn with the others given: the others hold what a twin launch with every
    # output gives, and the NULL one's bytes stay
    assert _launch(env, pol, K, {}, 1 << 23) == 0
    twin = _env(n, base_seed=9, max_steps=3)
    for k_ in (K - 1, K, K):
        fused(twin, pol, k_, 1 << 23)
    for name in KEYS:
        before = raw.clone()
        assert _launch(env, pol, 2, {k: v for k, v in ptrs.items() if k != name}, 1 << 23) == 0, name
        torch.cuda.synchronize()
        exp = fused(twin, pol, 2, 1 << 23)
        off, size = at[name]
        assert torch.equal(raw[off:off + size], before[off:off + size]), f"{name}: written though NULL"
        for other in KEYS:
            if other != name:
                o2, s2 = at[other]
                rows = s2 if other in per_env else s2 // K * 2
                assert torch.equal(raw[o2:o2 + rows], exp[other].reshape(-1).view(torch.uint8)), (name, other)
        assert bool((raw[~within] == 0xA5).all())
        _state_equal(name, env, twin)
    assert torch.equal(rng_before[:, 12:24], env.get_state()[2][:, 12:24])
    assert env.policy_step == (K - 1) + K + K + 2 * len(KEYS) and env.error_count() == 0
    env.close()
    twin.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------
def test_preview_rollout_refusals():
    """Every refusal, in the header's order, through the check-only entry and through the launch: the status, nothing written,
    the counter unchanged; an earlier refusal wins over a later one."""
    import torch

    import marl_sortingenv_amd as M

    INVALID, UNSUPPORTED = -1, -2
    n, K = 64, 2
    pol = _actor("mono")
    opened = []

    def keep(e):
        opened.append(e)
        return e

    try:
        env = keep(_env(n))
        raw, at = guarded(_sizes(n, K))
        ptrs = {name: raw.data_ptr() + off for name, (off, _) in at.items()}
        assert _check_call(env, pol, K) == 0 and env.policy_step == 0  # the check launches nothing
        assert _launch(env, pol, K, ptrs) == 0
        torch.cuda.synchronize()
        filled, state, t = raw.clone(), [x.clone() for x in env.get_state()], env.policy_step
        OUT_ONLY = ("struct_size", "no_out", "ptrs")

        def refused(status, e=env, p=pol, k=K, message=None, **kw):
            """The check-only entry first: only a call it refuses is sent to the entry that could launch."""
            if not any(key in kw for key in OUT_ONLY):
                assert _check_call(e, p, k, **kw) == status
                assert message is None or message in env.L.mse_last_error(), env.L.mse_last_error()
            before = e.policy_step
            where = kw.pop("ptrs", ptrs)
            assert _launch(e, p, k, where, **kw) == status
            assert message is None or message in env.L.mse_last_error(), env.L.mse_last_error()
            torch.cuda.synchronize()
            assert torch.equal(raw, filled), "a refused call wrote to the buffers"
            assert e.policy_step == before

        # MSE_ERR_INVALID_ARGUMENT, in the header's order
        assert env.L.mse_rollout_policy_preview_check(None, pol._h, K, SEED, MIX_SEED, 0, 0) == INVALID
        refused(INVALID, p=None, message=b"NULL")
        refused(INVALID, no_out=True, message=b"NULL")
        refused(INVALID, struct_size=8, message=b"struct_size")
        refused(INVALID, struct_size=8, k=0, message=b"struct_size")  # the earlier refusal wins
        refused(INVALID, k=0, message=b"k_steps")
        refused(INVALID, k=-1, message=b"k_steps")
        press_env = keep(M.BatchedSortingEnv(kind="press", num_envs=n, device=0, auto_reset=True))
        refused(INVALID, e=press_env, p=_actor("press"), message=b"Env_3")
        refused(INVALID, e=keep(M.BatchedSortingEnv(kind="sort", num_envs=n, device=0, auto_reset=True)), message=b"Env_3")
        refused(INVALID, e=press_env, k=0, message=b"k_steps")
        refused(INVALID, p=_actor("press"), message=b"29 -> 22")
        refused(INVALID, p=_actor("sort"), threshold=ONE + 1, message=b"29 -> 22")
        if torch.cuda.device_count() > 1:
            refused(INVALID, p=M.MlpPolicy.random_init(29, 22, seed=1, device=1), message=b"different devices")
        refused(INVALID, threshold=ONE + 1, message=b"expert_threshold")
        refused(INVALID, threshold=0xFFFFFFFF, mix_seed=SEED, message=b"expert_threshold")
        for thr in (0, 1 << 23, ONE):
            refused(INVALID, mix_seed=SEED, threshold=thr, message=b"mix_seed")
        refused(INVALID, mix_seed=SEED, flags=1, message=b"mix_seed")
        for flag in (1, 4, 8, 16, 32, 64, 128, 256, 512, 2048, 1 << 31):  # MSE_STEP_UNMASKED and every other foreign bit
            refused(INVALID, flags=flag, message=b"unknown rollout flag")
        no_auto = keep(_env(n, auto_reset=False))
        refused(INVALID, e=no_auto, message=b"auto_reset")
        refused(INVALID, e=no_auto, flags=1, message=b"unknown rollout flag")
        not_reset = keep(_env(n, reset_now=False))
        refused(INVALID, e=not_reset, message=b"before mse_reset")
        env.trace_begin(0, 16)
        refused(INVALID, message=b"trace")
        for cls in (M.FusedPolicyRollout, M.PolicyRolloutCollector):
            col = cls(env, pol, K, seed=SEED, view="preview")
            if cls is M.FusedPolicyRollout:
                with pytest.raises(M.MseError) as err:
                    col.collect()
                assert err.value.status == INVALID
        env.trace_end()
        for name in ("observations", "action_masks"):
            refused(INVALID, ptrs=dict(ptrs, **{name: ptrs[name] + 4}), message=b"16-byte aligned")
        env.trace_begin(0, 16)
        refused(INVALID, ptrs=dict(ptrs, observations=ptrs["observations"] + 4), message=b"trace")
        env.trace_end()
        # MSE_ERR_UNSUPPORTED_CONFIG
        literal = keep(_env(n, literal_choice=True))
        refused(UNSUPPORTED, e=literal, message=b"literal_choice")
        refused(INVALID, e=literal, ptrs=dict(ptrs, action_masks=ptrs["action_masks"] + 1), message=b"16-byte aligned")
        gen_env = keep(_env(n, config=M.SortingEnvConfig().with_overrides(GEN)))
        refused(UNSUPPORTED, e=gen_env, message=b"general generator mode")
        # tables that do not fit (tests/test_gpu_demo_rollout.py: about 56 KB of them): served in 32-env waves, refused in
        # 64-env waves - 21 264 B of weights + 8 x 12 544 B of wave tiles + the tables > 160 KiB
        big_cfg = M.SortingEnvConfig().with_overrides(BIG_TABLES)
        small_big = keep(_env(n, config=big_cfg))
        assert _check_call(small_big, pol, K) == 0
        big = keep(_env(256 * cus() + 1, config=big_cfg))
        big_state = [x.clone() for x in big.get_state()]
        big_bufs = _buffers(big.num_envs, K, ("rewards", "last_dones"))
        assert _check_call(big, pol, K) == UNSUPPORTED and b"LDS image does not fit" in big.L.mse_last_error()
        assert _launch(big, pol, K, {k: v.data_ptr() for k, v in big_bufs.items()}) == UNSUPPORTED
        torch.cuda.synchronize()
        assert not bool(big_bufs["rewards"].any()) and big.policy_step == 0
        for x, y in zip(big_state, big.get_state()):
            assert torch.equal(x, y)
        # the env the refusals were tried on is where it was
        for x, y in zip(state, env.get_state()):
            assert torch.equal(x, y)
        assert env.policy_step == t
        assert _check_call(env, pol, K, ONE, CHECK_OVERFLOW | DETERMINISTIC) == 0
        # the served big-table handle gives the hand loop's rows
        hand = hand_collect(keep(_env(n, config=big_cfg)), pol, K)
        bits_equal("big tables, 32-env waves", fused(small_big, pol, K), hand, KEYS)
    finally:
        for e in opened:
            e.close()
