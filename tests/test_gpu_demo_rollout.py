"""GPU: the fused demonstration rollout (mse_rollout_demo, FusedDemonstrationRollout) - the rule-based controller
labelling every state a student, the expert or a mixture of the two visits, K steps per launch - against

  * its multi-launch twin DemonstrationCollector (copies, mse_rule_actions, MlpPolicy.forward, mse_step) at beta = 0
    (the student steps) and, without an actor, beta = 1: bit for bit, every buffer, the full state and the policy step
    counter after every launch, at both wave shapes and both precision forms;
  * the sentence of include/mse.h written out in this file (`hand_collect`: rule, forward, the numpy who-steps rule of
    tests/test_demo_mixture_cpu.py, step) for the mixture and for check_overflow, which the twin does not offer;
  * guard bytes, NULL outputs, untouched streams, every refusal with its check-only form, and the learner's loop.

All comparisons are on bits.  max_steps = 3 puts episode ends inside and across the launches."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests.rollout_checks import bits_equal, cus, guarded, inside, lib, overflow_config
from tests.test_demo_mixture_cpu import MIX_SEED, ONE, who_steps
from tests.test_gpu_model_rollout import _state_equal

pytestmark = pytest.mark.gpu

SEED = 77
KEYS = ("observations", "action_masks", "actions", "stepped_actions", "rewards", "episode_starts", "last_dones", "returns")
DIMS = {"sort": (13, 2), "press": (16, 11), "mono": (29, 22)}
SNAP_CURRENT_STEP = 32  # column of mse_get_state's integer record that holds the env's current_step
LAUNCHES = (5, 1, 4)
GAMMA = 0.97


def _env(kind, n, noise=0.05, max_steps=3, base_seed=11, **kw):
    import marl_sortingenv_amd as M

    kw.setdefault("auto_reset", True)
    return M.BatchedSortingEnv(kind=kind, num_envs=n, device=0, base_seed=base_seed, max_steps=max_steps,
                               noise_sorting=noise, balesize=200, **kw)


@functools.lru_cache(maxsize=None)
def _actor(kind, precision="f16x3", head_gain=20.0, seed=3):
    """An untrained student of the env's own dimensions, its action head scaled up so that the draws and the argmax
    matter (SB3's initial 0.01 leaves the logits within ~1e-2 of each other); built once, never changed."""
    import marl_sortingenv_amd as M
    from marl_sortingenv_amd.policy import _shapes

    d, a = DIMS[kind]
    w = dict(M.MlpPolicy.random_init(d, a, seed=seed, precision=precision).weights)
    w["action_net.weight"] = w["action_net.weight"] * np.float32(head_gain)
    p = M.MlpPolicy(d, a, {k: v.reshape(sh) for (k, v), sh in zip(w.items(), _shapes(d, a))}, precision=precision)
    assert p.precision == precision
    return p


def hand_collect(env, K, actor=None, seed=SEED, mix_seed=MIX_SEED, threshold=ONE, deterministic=False,
                 check_overflow=False, gamma=GAMMA):
    """K rounds of: read obs and mask, mse_rule_actions, mse_policy_forward(seed, t = the handle's counter, index_offset =
    the env's), the who-steps rule in numpy, mse_step.  -> the collectors' dict plus `expert_stepped`."""
    import torch

    from marl_sortingenv_amd._lib import check
    from marl_sortingenv_amd.learner import _ptr, _stream

    n, dev = env.num_envs, env.device
    f32, i32, u8 = torch.float32, torch.int32, torch.uint8
    b = {"observations": torch.empty((K, n, env.obs_dim), dtype=f32, device=dev),
         "action_masks": torch.empty((K, n, env.num_actions), dtype=u8, device=dev),
         "actions": torch.empty((K, n), dtype=i32, device=dev), "stepped_actions": torch.empty((K, n), dtype=i32, device=dev),
         "expert_stepped": torch.empty((K, n), dtype=u8, device=dev), "rewards": torch.empty((K, n), dtype=f32, device=dev),
         "episode_starts": torch.empty((K, n), dtype=u8, device=dev), "returns": torch.empty((K, n), dtype=f32, device=dev)}
    env.refresh_outputs()  # env.obs / env.mask of the current state, whatever ran on the handle before
    last_done = (env.get_state()[0][:, SNAP_CURRENT_STEP] == 0).to(u8)
    for k in range(K):
        t = env.policy_step
        b["observations"][k].copy_(env.obs)
        b["action_masks"][k].copy_(env.mask)
        b["episode_starts"][k].copy_(last_done)
        rule = env.rule_actions()
        b["actions"][k].copy_(rule)
        if actor is None:
            who = np.ones(n, dtype=np.uint8)
            stepped = rule
        else:
            a = actor.forward(env.obs, env.mask, seed=seed, t=t, deterministic=deterministic, index_offset=env.index_offset)["action"]
            who = who_steps(n, env.index_offset, mix_seed, t, threshold)
            stepped = torch.where(torch.from_numpy(who).to(dev) != 0, rule, a)
        b["expert_stepped"][k].copy_(torch.from_numpy(who))
        b["stepped_actions"][k].copy_(stepped)
        _, rew, done, _ = env.step(b["stepped_actions"][k], check_overflow=check_overflow)
        b["rewards"][k].copy_(rew)
        last_done = done.clone()
    b["last_dones"] = last_done
    zeros = torch.zeros((K + 1, n), dtype=f32, device=dev)
    adv = torch.empty((K, n), dtype=f32, device=dev)
    check(env.L.mse_gae(K, n, _ptr(b["rewards"]), _ptr(zeros), _ptr(b["episode_starts"]), _ptr(zeros[K]), _ptr(last_done),
                        gamma, 1.0, _ptr(adv), _ptr(b["returns"]), _stream(dev)))
    return b


# ---- 1. fused == DemonstrationCollector, bit for bit --------------------------------------------------------------------
ACTORS = {
    "expert": dict(actor=None),
    "sampled_f16x3": dict(actor="f16x3", deterministic=False),
    "argmax_f16x3": dict(actor="f16x3", deterministic=True),
    "sampled_f32": dict(actor="f32", deterministic=False),
    "argmax_f32": dict(actor="f32", deterministic=True),
}


def _compare_with_twin(tag, kind, n, noise, max_steps, mode, launches=LAUNCHES, **kw):
    import marl_sortingenv_amd as M

    precision = ACTORS[mode]["actor"]
    actor = None if precision is None else _actor(kind, precision)
    det = ACTORS[mode].get("deterministic", False)
    a, b = _env(kind, n, noise, max_steps, **kw), _env(kind, n, noise, max_steps, **kw)
    last_dones, n_done, differs = None, 0, 0
    for K in launches:
        t0 = a.policy_step
        fused = M.FusedDemonstrationRollout(a, K, actor=actor, deterministic_actor=det, gamma=GAMMA, seed=SEED, mix_seed=MIX_SEED)
        assert fused.beta == (1.0 if actor is None else 0.0)
        twin = M.DemonstrationCollector(b, K, actor=actor, deterministic_actor=det, gamma=GAMMA, seed=SEED)
        if last_dones is None:
            assert twin.t == b.policy_step == 0  # a fresh env: the twin's own t and the handle's counter agree
        else:  # a stepped handle: the twin carries t and the last dones itself
            twin.t = b.policy_step
            twin._last_done.copy_(last_dones)
        got, exp = fused.collect(), twin.collect()
        bits_equal(f"{tag} K={K}", got, exp, KEYS)
        _state_equal(f"{tag} K={K}", a, b)
        assert a.policy_step == t0 + K
        assert bool((got["expert_stepped"] == (1 if actor is None else 0)).all())
        last_dones = exp["last_dones"]
        n_done += int(got["episode_starts"][1:].sum()) + int(got["last_dones"].sum())
        differs += int((got["actions"] != got["stepped_actions"]).sum())
    assert a.error_count() == 0
    a.close()
    b.close()
    return n_done, differs


@pytest.mark.parametrize("mode", list(ACTORS))
@pytest.mark.parametrize("n", [1, 33, 257])
@pytest.mark.parametrize("kind", ["sort", "press", "mono"])
def test_fused_demo_rollout_matches_twin(kind, n, mode):
    """A lone lane, a ragged second tile, a second workgroup (or wave) with one env; launches of 5, 1 and 4 steps on the
    same handles; noise off and on; episodes that end inside the window (max_steps 3) and ones that do not (40)."""
    for noise in (0.0, 0.05):
        for max_steps in (3, 40):
            n_done, differs = _compare_with_twin(f"{kind} n={n} {mode} noise={noise} max_steps={max_steps}", kind, n, noise,
                                                 max_steps, mode)
            assert n_done >= (3 * n if max_steps == 3 else 0)
            if mode == "expert":
                assert differs == 0
            elif n > 1 and kind != "press":  # (early in an episode nothing can be pressed: the mask leaves one action)
                assert differs > 0, "an untrained actor does not act like the expert"


@pytest.mark.parametrize("mode", ["expert", "sampled_f16x3", "sampled_f32"])
def test_fused_demo_rollout_matches_twin_in_64_env_waves(mode):
    """256 x CUs + 1 envs: the smallest batch plan_policy_plain gives two tiles per wave in the f16x3 form."""
    _compare_with_twin(f"tiles=2 {mode}", "mono", 256 * cus() + 1, 0.05, 3, mode, launches=(2,))


def test_fused_demo_rollout_on_a_shard():
    """index_offset enters both stream keys: a shard's rows are the twin's, and its who-steps draws its own."""
    import marl_sortingenv_amd as M

    _compare_with_twin("index_offset", "mono", 33, 0.05, 3, "sampled_f16x3", index_offset=1000)
    n, K, off = 33, 4, 2 ** 32 + 5
    env = _env("mono", n, index_offset=off)
    b = M.FusedDemonstrationRollout(env, K, actor=_actor("mono"), beta=0.5, seed=SEED, mix_seed=MIX_SEED).collect()
    want = np.stack([who_steps(n, off, MIX_SEED, t, 1 << 23) for t in range(K)])
    assert np.array_equal(b["expert_stepped"].cpu().numpy(), want)
    env.close()


@pytest.mark.parametrize("kind", ["press", "mono"])
@pytest.mark.parametrize("mode", ["expert", "sampled_f16x3"])
def test_fused_demo_rollout_check_overflow(kind, mode):
    """check_overflow at container capacity 30, against the hand loop (the twin steps without it): episodes end by
    overflow with the termination penalty as the reward."""
    import marl_sortingenv_amd as M
    from marl_sortingenv_amd.config import SortingEnvConfig

    pen = np.float32(SortingEnvConfig().overflow_termination_penalty)
    actor = None if mode == "expert" else _actor(kind)
    for n in (33, 257):
        for noise in (0.0, 0.05):
            cfg = overflow_config(noise)
            a, b = _env(kind, n, noise, config=cfg), _env(kind, n, noise, config=cfg)
            hits = 0
            for K in LAUNCHES:
                fused = M.FusedDemonstrationRollout(a, K, actor=actor, gamma=GAMMA, seed=SEED, mix_seed=MIX_SEED, check_overflow=True)
                got = fused.collect()
                exp = hand_collect(b, K, actor, threshold=ONE if actor is None else 0, check_overflow=True)
                bits_equal(f"{kind} {mode} n={n} noise={noise} K={K}", got, exp, KEYS + ("expert_stepped",))
                _state_equal(f"{kind} {mode} n={n} noise={noise} K={K}", a, b)
                hits += int((got["rewards"] == float(pen)).sum())
            assert hits >= 1, "no episode ended by overflow"
            a.close()
            b.close()


# ---- 2. the mixture ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deterministic", [False, True], ids=["sampled", "argmax"])
@pytest.mark.parametrize("n", [33, 257])
@pytest.mark.parametrize("kind", ["sort", "press", "mono"])
def test_mixture_matches_the_hand_loop(kind, n, deterministic):
    """Threshold 2^23, mix_seed 99, t = 0 .. 9 (tests/test_demo_mixture_cpu.py asserts that the expert's share is between
    40 % and 60 % at both sizes): every buffer, the state and the counter are the hand loop's, `expert_stepped` is the
    numpy restatement, and both branches were taken with different actions."""
    import torch

    import marl_sortingenv_amd as M

    actor = _actor(kind)
    a, b = _env(kind, n), _env(kind, n)
    t = 0
    for K in LAUNCHES:
        fused = M.FusedDemonstrationRollout(a, K, actor=actor, deterministic_actor=deterministic, beta=0.5, gamma=GAMMA,
                                            seed=SEED, mix_seed=MIX_SEED)
        got = fused.collect()
        exp = hand_collect(b, K, actor, threshold=1 << 23, deterministic=deterministic)
        bits_equal(f"{kind} n={n} K={K}", got, exp, KEYS + ("expert_stepped",))
        _state_equal(f"{kind} n={n} K={K}", a, b)
        want = np.stack([who_steps(n, 0, MIX_SEED, t + k, 1 << 23) for k in range(K)])
        assert np.array_equal(got["expert_stepped"].cpu().numpy(), want)
        es = got["expert_stepped"] != 0
        assert torch.equal(got["stepped_actions"][es], got["actions"][es])  # where the expert steps, the label is stepped
        if K == 5:
            assert bool(es.any()) and bool((~es).any())
            if kind != "press":  # (early in an episode nothing can be pressed: the mask leaves one action)
                assert bool((got["stepped_actions"][~es] != got["actions"][~es]).any()), "the student never differs from the expert"
        t += K
    assert a.policy_step == t == 10
    a.close()
    b.close()


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
@pytest.mark.parametrize("n", [33, 257])
def test_mixture_ends(n, precision):
    """Threshold 0 equals the actor-only run; threshold 2^24 equals the actor=None run in every buffer (there
    `expert_stepped` is all ones from the rule itself, here from the comparison); the counter advances by K in each; an
    untrained actor's stepped rows differ from the labels somewhere."""
    import marl_sortingenv_amd as M

    K, kind = 6, "mono"
    actor = _actor(kind, precision)
    envs = [_env(kind, n) for _ in range(4)]
    zero = M.FusedDemonstrationRollout(envs[0], K, actor=actor, beta=0.0, gamma=GAMMA, seed=SEED, mix_seed=MIX_SEED).collect()
    twin = M.DemonstrationCollector(envs[1], K, actor=actor, gamma=GAMMA, seed=SEED).collect()
    bits_equal("threshold 0", zero, twin, KEYS)
    _state_equal("threshold 0", envs[0], envs[1])
    assert not bool(zero["expert_stepped"].any())
    assert bool((zero["stepped_actions"] != zero["actions"]).any()), "an untrained actor does not act like the expert"
    one = M.FusedDemonstrationRollout(envs[2], K, actor=actor, beta=1.0, gamma=GAMMA, seed=SEED, mix_seed=MIX_SEED).collect()
    none = M.FusedDemonstrationRollout(envs[3], K, actor=None, gamma=GAMMA).collect()
    bits_equal("threshold 2^24", one, none, KEYS + ("expert_stepped",))
    _state_equal("threshold 2^24", envs[2], envs[3])
    assert bool((one["expert_stepped"] == 1).all()) and bool((one["stepped_actions"] == one["actions"]).all())
    assert all(e.policy_step == K for e in envs)
    for e in envs:
        e.close()


def test_beta_is_settable_between_calls():
    import marl_sortingenv_amd as M

    n, K = 257, 4
    env = _env("mono", n)
    fused = M.FusedDemonstrationRollout(env, K, actor=_actor("mono"), beta=1.0, seed=SEED, mix_seed=MIX_SEED)
    shares = []
    for beta in (1.0, 0.25, 0.0):
        fused.beta = beta
        assert fused.beta == beta
        t0 = env.policy_step
        b = fused.collect()
        want = np.stack([who_steps(n, 0, MIX_SEED, t0 + k, M.expert_threshold(beta)) for k in range(K)])
        assert np.array_equal(b["expert_stepped"].cpu().numpy(), want)
        shares.append(float(want.mean()))
    assert shares[0] == 1.0 and 0.15 < shares[1] < 0.35 and shares[2] == 0.0
    for bad in (float("nan"), -0.1, 1.5):
        with pytest.raises(ValueError):
            fused.beta = bad
    assert fused.beta == 0.0
    with pytest.raises(ValueError):
        M.FusedDemonstrationRollout(env, K, actor=None, beta=0.5)
    with pytest.raises(ValueError):
        M.FusedDemonstrationRollout(env, K, actor=None).beta = 0.0
    with pytest.raises(ValueError):
        M.FusedDemonstrationRollout(env, K, actor=_actor("mono"), seed=5, mix_seed=5)
    with pytest.raises(ValueError):
        M.FusedDemonstrationRollout(env, K, actor=_actor("press"))
    with pytest.raises(ValueError):
        M.FusedDemonstrationRollout(env, 0)
    env.close()


# ---- 3. memory ------------------------------------------------------------------------------------------------------------------
def _sizes(kind, n, K):
    d, a = DIMS[kind]
    return {"observations": K * n * d * 4, "action_masks": K * n * a, "episode_starts": K * n, "labels": K * n * 4,
            "stepped_actions": K * n * 4, "expert_stepped": K * n, "rewards": K * n * 4, "last_dones": n}


def _raw_call(env, actor, K, flags, ptrs, seed=SEED, mix_seed=MIX_SEED, threshold=1 << 23, struct_size=None, no_out=False):
    from marl_sortingenv_amd._lib import DEMO_BUFFER_NAMES, MseDemoBuffers

    out = MseDemoBuffers(C.sizeof(MseDemoBuffers) if struct_size is None else struct_size, 0,
                         *(ptrs.get(name) for name in DEMO_BUFFER_NAMES))
    return lib().mse_rollout_demo(None if env is None else env._h, None if actor is None else actor._h, K, seed, mix_seed,
                                  threshold, flags, None if no_out else C.byref(out), None)


def _check_call(env, actor, K, flags=0, seed=SEED, mix_seed=MIX_SEED, threshold=1 << 23):
    return lib().mse_rollout_demo_check(None if env is None else env._h, None if actor is None else actor._h, K, seed,
                                        mix_seed, threshold, flags)


@pytest.mark.parametrize("with_actor", [True, False], ids=["actor", "expert"])
@pytest.mark.parametrize("kind", ["sort", "press", "mono"])
def test_fused_demo_rollout_memory(kind, with_actor):
    """97 envs (a ragged wave whose rows leave through the scalar path): no guard byte is written, each output may be
    NULL, and the label consumes no draw - the rng_pressing and rng_sorting streams (words 12-23 of the RNG record),
    which no step reads, are where they were."""
    import torch

    from marl_sortingenv_amd._lib import DEMO_BUFFER_NAMES

    n, K = 97, 4
    actor = _actor(kind) if with_actor else None
    env = _env(kind, n, base_seed=9)
    rng_before = env.get_state()[2].clone()
    raw, at = guarded(_sizes(kind, n, K))
    ptrs = {name: raw.data_ptr() + off for name, (off, _) in at.items()}
    assert _raw_call(env, actor, K, 0, ptrs) == 0
    torch.cuda.synchronize()
    within = inside(raw, at)
    assert bool((raw[~within] == 0xA5).all()), "a guard byte was written"
    first = raw.clone()
    twin = _env(kind, n, base_seed=9)
    exp = hand_collect(twin, K, actor, threshold=1 << 23)
    for name, key in (("observations", "observations"), ("action_masks", "action_masks"), ("labels", "actions"),
                      ("stepped_actions", "stepped_actions"), ("expert_stepped", "expert_stepped"), ("rewards", "rewards"),
                      ("episode_starts", "episode_starts"), ("last_dones", "last_dones")):
        off, size = at[name]
        assert torch.equal(raw[off:off + size], exp[key].contiguous().view(torch.uint8).reshape(-1)), name
    rng_after = env.get_state()[2]
    assert torch.equal(rng_before[:, 12:24], rng_after[:, 12:24])
    assert torch.equal(rng_after, twin.get_state()[2])
    # every output NULL, then one at a time
    assert _raw_call(env, actor, K, 0, {}) == 0
    for name in DEMO_BUFFER_NAMES:
        assert _raw_call(env, actor, 1, 0, {name: ptrs[name]}) == 0, name
    torch.cuda.synchronize()
    assert bool((raw[~within] == 0xA5).all())
    assert not torch.equal(raw, first)  # (the single outputs were rewritten)
    assert env.policy_step == K + K + len(DEMO_BUFFER_NAMES) and env.error_count() == 0
    env.close()
    twin.close()


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------
# the table image grows with container_capacity (one 4-byte level per unit): at 12 000 it is about 56 KB, which
# mse_create accepts (below 64 KiB) and which leaves the 32-env waves room (21 264 B of weights + 8 x 6 272 B of wave
# tiles + the tables < 160 KiB) and not the 64-env waves (21 264 + 8 x 12 544 + more than 48 004 B > 160 KiB)
BIG_TABLES = {"pressing_station": {"container_capacity": 12000}}
GEN = {"simulation": {"input_batch_size": 90}}


def test_fused_demo_rollout_refusals():
    import torch

    import marl_sortingenv_amd as M

    INVALID, UNSUPPORTED = -1, -2
    kind, n, K = "mono", 64, 2
    actor = _actor(kind)
    opened = []

    def keep(e):
        opened.append(e)
        return e

    try:
        env = keep(_env(kind, n))
        raw, at = guarded(_sizes(kind, n, K))
        ptrs = {name: raw.data_ptr() + off for name, (off, _) in at.items()}
        assert _check_call(env, actor, K) == 0 and env.policy_step == 0  # the check launches nothing
        assert _raw_call(env, actor, K, 0, ptrs) == 0
        torch.cuda.synchronize()
        filled, state, t = raw.clone(), [x.clone() for x in env.get_state()], env.policy_step

        def refused(status, e=env, a=actor, k=K, flags=0, p=None, check_too=True, **kw):
            """The check-only entry first (same status, same message), then the entry that could launch."""
            msg = None
            if check_too:
                assert _check_call(e, a, k, flags, **kw) == status
                msg = env.L.mse_last_error()
            before = None if e is None else e.policy_step
            assert _raw_call(e, a, k, flags, ptrs if p is None else p, **kw) == status
            assert msg is None or env.L.mse_last_error() == msg
            torch.cuda.synchronize()
            assert torch.equal(raw, filled), "a refused call wrote to the buffers"
            assert before is None or e.policy_step == before

        refused(INVALID, e=None)
        assert _raw_call(env, actor, K, 0, ptrs, no_out=True) == INVALID
        assert _raw_call(env, actor, K, 0, ptrs, struct_size=8) == INVALID
        refused(INVALID, k=0)
        refused(INVALID, k=-1)
        refused(INVALID, a=_actor("press"))
        refused(INVALID, a=_actor("sort"))
        refused(INVALID, threshold=ONE + 1)
        refused(INVALID, threshold=2 ** 32 - 1)
        refused(INVALID, a=None, threshold=ONE + 1)
        refused(INVALID, seed=7, mix_seed=7)
        assert _check_call(env, None, K, seed=7, mix_seed=7) == 0  # without an actor neither seed selects anything
        for flag in (1, 4, 8, 16, 32, 64, 128, 256, 1024, 1 << 31):  # MSE_STEP_UNMASKED and every bit that is not one of the two
            refused(INVALID, flags=flag)
        assert _check_call(env, actor, K, flags=2 | 512) == 0
        refused(INVALID, e=keep(_env(kind, n, auto_reset=False)))
        refused(INVALID, e=keep(_env(kind, n, reset_now=False)))
        env.trace_begin(0, 16)
        refused(INVALID)
        with pytest.raises(M.MseError) as err:
            M.FusedDemonstrationRollout(env, K, actor=actor).collect()
        assert err.value.status == INVALID
        env.trace_end()
        for name in ("observations", "action_masks"):  # the 16-byte rule
            refused(INVALID, p=dict(ptrs, **{name: ptrs[name] + 4}), check_too=False)
        cfg = M.SortingEnvConfig()
        refused(UNSUPPORTED, e=keep(_env(kind, n, literal_choice=True)))
        gen_env = keep(_env(kind, n, config=cfg.with_overrides(GEN)))
        refused(UNSUPPORTED, e=gen_env)
        # tables that do not fit: the same config is served in 32-env waves and refused in 64-env waves
        big_cfg = cfg.with_overrides(BIG_TABLES)
        small_big = keep(_env(kind, n, config=big_cfg))
        assert _check_call(small_big, actor, K) == 0
        assert _raw_call(small_big, actor, K, 0, ptrs) == 0
        torch.cuda.synchronize()
        filled = raw.clone()
        big = keep(_env(kind, 256 * cus() + 1, config=big_cfg))
        big_state = [x.clone() for x in big.get_state()]
        refused(UNSUPPORTED, e=big)
        assert b"LDS image does not fit" in big.L.mse_last_error()
        for x, y in zip(big_state, big.get_state()):
            assert torch.equal(x, y)
        assert big.policy_step == 0 and gen_env.policy_step == 0
        with pytest.raises(M.MseError) as err:
            M.FusedDemonstrationRollout(gen_env, K, actor=actor).collect()
        assert err.value.status == UNSUPPORTED
        # the env the refusals were tried on is where it was, and still serves
        for x, y in zip(state, env.get_state()):
            assert torch.equal(x, y)
        assert env.policy_step == t
        assert M.FusedDemonstrationRollout(env, K, actor=actor).collect()["rewards"].shape == (K, n)
    finally:
        for e in opened:
            e.close()


# ---- 5. the learner -------------------------------------------------------------------------------------------------------------
class _HandCollector:
    """`hand_collect` behind the collectors' surface: `beta` is written by the learner before each `collect()`."""

    def __init__(self, env, K, actor):
        self.env, self.K, self.actor, self.beta = env, K, actor, 1.0

    def collect(self):
        import marl_sortingenv_amd as M

        return hand_collect(self.env, self.K, self.actor, threshold=M.expert_threshold(self.beta), gamma=0.99)


def test_learner_with_a_beta_schedule_is_the_hand_loop():
    """ImitationLearner.learn(fused, 2 iterations, beta=lambda f: 1 - f): beta 1 then 0.5; records and weights are those
    of the same loop over the hand-written collection, bit for bit, and a record's expert share is the buffer's mean."""
    import torch

    import marl_sortingenv_amd as M
    from tests.ppo_checks import make_policy, same_bits

    n, K = 64, 8
    seen = []
    out = []
    for which in ("fused", "hand"):
        pol, _ = make_policy(29, 22, 71, precision="f32")
        learner = M.ImitationLearner(pol, learning_rate=1e-3, n_epochs=2, batch_size=100, seed=5)
        env = _env("mono", n, max_steps=5)
        if which == "fused":
            col = M.FusedDemonstrationRollout(env, K, actor=pol, seed=SEED, mix_seed=MIX_SEED)
            cb = lambda it, rec, col=col: seen.append((col.beta, float(col.buffers["expert_stepped"].float().mean())))
        else:
            col, cb = _HandCollector(env, K, pol), None
        hist = learner.learn(col, 2, beta=lambda f: 1.0 - f, callback=cb)
        torch.cuda.synchronize()
        out.append((hist, learner.weights.clone(), learner.m.clone(), learner.v.clone(), env.get_state()))
        env.close()
    (hf, wf, mf, vf, sf), (hh, wh, mh, vh, sh) = out
    assert hf == hh, "the records differ"
    assert same_bits(wf, wh) and same_bits(mf, mh) and same_bits(vf, vh)
    for x, y in zip(sf, sh):
        assert torch.equal(x, y)
    assert [r["beta"] for r in hf] == [1.0, 0.5] and [b for b, _ in seen] == [1.0, 0.5]
    assert [r["expert_share"] for r in hf] == [s for _, s in seen]
    assert hf[0]["expert_share"] == 1.0 and 0.4 < hf[1]["expert_share"] < 0.6
    want = np.stack([who_steps(n, 0, MIX_SEED, K + k, 1 << 23) for k in range(K)])
    assert hf[1]["expert_share"] == float(torch.from_numpy(want).float().mean())
    # a number serves as well; None leaves the collector's beta and the records alone
    pol, _ = make_policy(29, 22, 71, precision="f32")
    env = _env("mono", n, max_steps=5)
    col = M.FusedDemonstrationRollout(env, K, actor=pol, beta=0.25, seed=SEED, mix_seed=MIX_SEED)
    learner = M.ImitationLearner(pol, n_epochs=1, batch_size=256, seed=5)
    rec = learner.learn(col, 1)[0]
    assert "beta" not in rec and "expert_share" not in rec and col.beta == 0.25
    rec = learner.learn(col, 1, beta=0.75)[0]
    assert rec["beta"] == 0.75 and col.beta == 0.75 and 0.65 < rec["expert_share"] < 0.85
    env.close()
