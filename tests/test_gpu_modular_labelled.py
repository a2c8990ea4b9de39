"""GPU: the labelled modular collection (mse_rollout_modular_labelled, FusedModularRollout(expert_labels=True)) - both
agents, the rule-based controller's label in its two halves and DAgger's who-steps mixture in one launch - against

  * the plain FusedModularRollout at beta = 0: every mse_modular_buffers key, the state and the step counter, bit for bit;
  * its multi-launch twin ModularRolloutCollector(expert_labels=True) at beta 0, 0.5 and 1: every twin key and the four
    label keys, the state, and expert_stepped against mse_demo_who_steps_host row by row;
  * a hand replay of the stepped actions with rule_actions() before each step (tests/test_gpu_labelled_rollout.py's
    hand_labels);
  * DemonstrationCollector(agent="sort" | "press", actor=None) at beta = 1, which demo_view replaces;
  * a shard, the deterministic flags and check_overflow, guard bytes, NULL outputs, the untouched rng planes, and every
    refusal in the header's order.

All comparisons are on bits.  max_steps = 3 puts episode ends inside and across the launches."""
import ctypes as C

import numpy as np
import pytest

from tests import replay
from tests.rollout_checks import bits_equal, cus, guarded, inside, overflow_config, who_host
from tests.test_gpu_labelled_rollout import hand_labels
from tests.test_gpu_model_rollout import _state_equal
from tests.test_gpu_modular_rollout import (BIG_TABLES_META, GEN_META, MODES, PRESS_SEED, SORT_SEED, TWIN_KEYS, _dones, _env, _pair,
                                            _sizes)

pytestmark = pytest.mark.gpu

MIX_SEED = 2026
ONE = 1 << 24
LABEL_KEYS = ("sort_expert_actions", "press_expert_actions", "stepped_actions", "expert_stepped")
PLAIN_KEYS = TWIN_KEYS + ("rewards_sort", "rewards_press")  # every member of mse_modular_buffers
LAUNCHES = (5, 1, 4)


def _labelled(cls, env, K, press_masked=True, beta=0.0, **kw):
    return cls(env, *_pair(), K, SORT_SEED, PRESS_SEED, press_masked=press_masked, expert_labels=True, beta=beta,
               mix_seed=MIX_SEED, **kw)


def _label_rows_consistent(b, K):
    """What holds for every labelled rollout, whoever stepped: the halves are in range, and stepped_actions is the label
    where the expert stepped and 11 sort + press where the pair did."""
    import torch

    s, p = b["sort_expert_actions"][:K], b["press_expert_actions"][:K]
    assert bool(((s >= 0) & (s <= 1) & (p >= 0) & (p <= 10)).all())
    who = b["expert_stepped"][:K] != 0
    want = torch.where(who, 11 * s + p, 11 * b["sort_actions"][:K] + b["press_actions"][:K])
    assert torch.equal(b["stepped_actions"][:K], want)


# ---- 1. labelled at beta = 0 == the plain launch ------------------------------------------------------------------------
def _compare_with_plain(tag, n, noise, press_masked, launches, **kw):
    import marl_sortingenv_amd as M

    a, b = _env(n, noise, base_seed=11, **kw), _env(n, noise, base_seed=11, **kw)
    kmax = max(launches)
    lab = _labelled(M.FusedModularRollout, a, kmax, press_masked)
    plain = M.FusedModularRollout(b, *_pair(), kmax, SORT_SEED, PRESS_SEED, press_masked=press_masked)
    assert set(lab.buffers) == set(plain.buffers) | set(LABEL_KEYS)
    n_done = 0
    for K in launches:
        t0 = a.policy_step
        got, exp = lab.collect(K), plain.collect(K)
        bits_equal(f"{tag} K={K}", got, exp, PLAIN_KEYS, K)
        _state_equal(f"{tag} K={K}", a, b)
        assert a.policy_step == t0 + K
        assert not bool(got["expert_stepped"][:K].any())
        _label_rows_consistent(got, K)
        n_done += int(_dones(got, K).sum())
    assert a.error_count() == 0
    a.close()
    b.close()
    return n_done


@pytest.mark.parametrize("press_masked", [True, False], ids=["masked", "plain"])
@pytest.mark.parametrize("noise", [0.0, 0.05], ids=["n0", "n5"])
@pytest.mark.parametrize("n", [1, 33, 257])
def test_labelled_at_beta_0_is_the_plain_rollout(n, noise, press_masked):
    """A lone lane with mirror lanes, a second 32-env wave holding one env, a second workgroup holding one env; launches of
    5, 1 and 4 steps on the same handles, three-step episodes."""
    assert _compare_with_plain(f"n={n} noise={noise} masked={press_masked}", n, noise, press_masked, LAUNCHES) >= 2 * n


@pytest.mark.parametrize("noise", [0.0, 0.05], ids=["n0", "n5"])
def test_labelled_at_beta_0_is_the_plain_rollout_in_64_env_waves(noise):
    """256 x CUs + 1 envs: the smallest batch plan_policy_plain gives two tiles per wave."""
    _compare_with_plain("tiles=2", 256 * cus() + 1, noise, True, (2,))


# ---- 2. fused == twin ------------------------------------------------------------------------------------------------------
def _compare_with_twin(tag, n, noise, press_masked, beta, launches, mode="sampled", gamma=None, index_offset=0, **kw):
    import marl_sortingenv_amd as M

    kw = dict(kw, base_seed=11, index_offset=index_offset)
    a, b = _env(n, noise, **kw), _env(n, noise, **kw)
    kmax = max(launches)
    fused = _labelled(M.FusedModularRollout, a, kmax, press_masked, beta, gamma=gamma)
    twin = _labelled(M.ModularRolloutCollector, b, kmax, press_masked, beta, gamma=gamma)
    threshold = M.expert_threshold(beta)
    keys = TWIN_KEYS + LABEL_KEYS + (("returns",) if gamma is not None else ())
    shares, rows = [], []
    for K in launches:
        t0 = a.policy_step
        got, exp = fused.collect(K, **MODES[mode]), twin.collect(K, **MODES[mode])
        bits_equal(f"{tag} K={K}", got, exp, keys, K)
        _state_equal(f"{tag} K={K}", a, b)
        assert a.policy_step == t0 + K
        _label_rows_consistent(got, K)
        who = got["expert_stepped"][:K].cpu().numpy()
        for k in range(K):
            assert np.array_equal(who[k], who_host(a, MIX_SEED, t0 + k, threshold)), (tag, K, k)
        shares.append(who)
        rows.append({key: got[key][:K].clone() for key in PLAIN_KEYS[:11] + LABEL_KEYS} | {"last_dones": got["last_dones"].clone()})
    a.close()
    b.close()
    return float(np.concatenate(shares).mean()), rows


@pytest.mark.parametrize("beta", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("noise", [0.0, 0.05], ids=["n0", "n5"])
@pytest.mark.parametrize("n", [1, 33, 257])
def test_labelled_rollout_matches_twin(n, noise, beta):
    share, _ = _compare_with_twin(f"n={n} noise={noise} beta={beta}", n, noise, noise != 0.0, beta, LAUNCHES, gamma=0.99)
    if beta == 0.5:  # n = 1 too: under MIX_SEED the lone env's ten draws (t = 0 .. 9) hold four expert steps
        assert 0.0 < share < 1.0
    if beta in (0.0, 1.0):
        assert share == beta


@pytest.mark.parametrize("beta", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("noise", [0.0, 0.05], ids=["n0", "n5"])
def test_labelled_rollout_matches_twin_in_64_env_waves(noise, beta):
    """256 x CUs + 1 envs, two tiles per wave: the pair steps every env (beta 0, the label keys still against the twin), the
    mixture, and the label path on every step (beta 1)."""
    share, _ = _compare_with_twin(f"tiles=2 beta={beta}", 256 * cus() + 1, noise, True, beta, (2,))
    if beta == 0.5:
        assert 0.45 < share < 0.55  # 131 074 draws at one half
    else:
        assert share == beta


# ---- 3. the labels by hand ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", [0.0, 0.5, 1.0])
def test_labels_are_rule_actions_of_the_replayed_states(beta):
    import torch

    import marl_sortingenv_amd as M

    n, noise = 97, 0.05
    a, c = _env(n, noise, base_seed=23), _env(n, noise, base_seed=23)
    fused = _labelled(M.FusedModularRollout, a, max(LAUNCHES), True, beta)
    for K in LAUNCHES:
        got = fused.collect(K)
        rule = hand_labels(c, got["stepped_actions"][:K])
        assert torch.equal(got["sort_expert_actions"][:K], rule // 11) and torch.equal(got["press_expert_actions"][:K], rule % 11)
    _state_equal("replay", a, c)  # the step counter too: mse_step counts one per step, as the rollout does
    a.close()
    c.close()


# ---- 4. beta = 1: DemonstrationCollector -------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", [0.0, 0.05], ids=["n0", "n5"])
def test_demo_view_at_beta_1_is_the_demonstration_collector(noise):
    import torch

    import marl_sortingenv_amd as M

    n, K, gamma = 97, 7, 0.97
    a, b, c = (_env(n, noise, base_seed=31) for _ in range(3))
    fused = _labelled(M.FusedModularRollout, a, K, True, 1.0, gamma=gamma)
    demos = {"sort": M.DemonstrationCollector(b, K, agent="sort", actor=None, gamma=gamma),
             "press": M.DemonstrationCollector(c, K, agent="press", actor=None, gamma=gamma)}
    keys = ("observations", "actions", "stepped_actions", "rewards", "episode_starts", "last_dones", "returns")
    for launch in range(2):
        fused.collect()
        for who, demo in demos.items():
            exp, got = demo.collect(), fused.demo_view(who)
            assert set(got) == set(exp) | {"expert_stepped"}
            for key in keys + (("action_masks",) if who == "press" else ()):
                x, y = got[key], exp[key]
                assert x.shape == y.shape and x.dtype == y.dtype, (who, key)
                if x.dtype == torch.float32:
                    x, y = x.view(torch.int32), y.view(torch.int32)
                assert torch.equal(x, y), (launch, who, key)
            assert got["action_masks"] is None if who == "sort" else got["action_masks"] is fused.buffers["press_masks"]
            assert got["actions"] is fused.buffers[f"{who}_expert_actions"] and bool(got["expert_stepped"].all())
    for e in (b, c):
        for x, y in zip(a.get_state(), e.get_state()):
            assert torch.equal(x, y)
    for e in (a, b, c):
        e.close()


# ---- 5. labels worth learning from: 40-step episodes ---------------------------------------------------------------------------
def test_labels_in_long_episodes():
    """Both sorter labels occur, the press label takes several values, and some press labels are forbidden by the mask
    row recorded beside them (DESIGN 4.16's "unusable" share): n and the seed were chosen on the twin, whose buffers are
    asserted on first."""
    import marl_sortingenv_amd as M

    n, K, noise = 97, 40, 0.05
    a, b = _env(n, noise, base_seed=5, max_steps=40), _env(n, noise, base_seed=5, max_steps=40)
    exp = _labelled(M.ModularRolloutCollector, b, K, True, 0.5).collect()
    s, p = exp["sort_expert_actions"].cpu().numpy(), exp["press_expert_actions"].cpu().numpy()
    forbidden = exp["press_masks"].cpu().numpy()[np.arange(K)[:, None], np.arange(n)[None, :], p] == 0
    print(f"twin, {K * n} rows: sorter labels {np.bincount(s.ravel(), minlength=2).tolist()}, press labels "
          f"{np.bincount(p.ravel(), minlength=11).tolist()}, forbidden by the mask {forbidden.mean():.4f}")
    assert set(np.unique(s)) == {0, 1}
    assert len(np.unique(p)) >= 2
    assert forbidden.any()
    got = _labelled(M.FusedModularRollout, a, K, True, 0.5).collect()
    bits_equal("long episodes", got, exp, TWIN_KEYS + LABEL_KEYS, K)
    _state_equal("long episodes", a, b)
    a.close()
    b.close()


# ---- 6. a shard --------------------------------------------------------------------------------------------------------------
def test_labelled_rollout_on_a_shard():
    """33 envs at index_offset = 224 are rows 224..256 of the 257-env run: both agents' keys and the mix key take the global
    index."""
    import torch

    _, whole = _compare_with_twin("whole", 257, 0.05, True, 0.5, (5, 4))
    _, shard = _compare_with_twin("shard", 33, 0.05, True, 0.5, (5, 4), index_offset=224)
    for w, s in zip(whole, shard):
        for key in s:
            x = w[key][224:] if key == "last_dones" else w[key][:, 224:]
            assert torch.equal(x.contiguous().view(torch.uint8), s[key].contiguous().view(torch.uint8)), key


# ---- 7. the deterministic flags and check_overflow -----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [m for m in MODES if m != "sampled"])
@pytest.mark.parametrize("noise", [0.0, 0.05], ids=["n0", "n5"])
def test_labelled_rollout_modes_match_twin(noise, mode):
    kw = dict(config=overflow_config(noise)) if mode == "overflow" else {}
    share, rows = _compare_with_twin(f"noise={noise} {mode}", 257, noise, True, 0.5, LAUNCHES, mode=mode, **kw)
    assert 0.0 < share < 1.0
    if mode == "overflow":
        from marl_sortingenv_amd.config import SortingEnvConfig

        pen = float(np.float32(SortingEnvConfig().overflow_termination_penalty))
        assert sum(int((r["rewards"] == pen).sum()) for r in rows) >= 1, "no episode ended by overflow"


# ---- 8. memory ---------------------------------------------------------------------------------------------------------------
def _raw_call(env, sort_ag, press_ag, K, flags, ptrs, lptrs, sort_seed=SORT_SEED, press_seed=PRESS_SEED, mix_seed=MIX_SEED,
              threshold=1 << 23, struct_size=None, label_struct_size=None, no_out=False, no_labels=False):
    from marl_sortingenv_amd._lib import MODULAR_BUFFER_NAMES, MODULAR_LABEL_BUFFER_NAMES, MseModularBuffers, MseModularLabelBuffers

    out = MseModularBuffers(C.sizeof(MseModularBuffers) if struct_size is None else struct_size, 0,
                            *(ptrs.get(name) for name in MODULAR_BUFFER_NAMES))
    labels = MseModularLabelBuffers(C.sizeof(MseModularLabelBuffers) if label_struct_size is None else label_struct_size, 0,
                                    *(lptrs.get(name) for name in MODULAR_LABEL_BUFFER_NAMES))
    return env.L.mse_rollout_modular_labelled(None if env is None else env._h, None if sort_ag is None else sort_ag._h,
                                              None if press_ag is None else press_ag._h, K, sort_seed, press_seed, mix_seed,
                                              threshold, flags, None if no_out else C.byref(out),
                                              None if no_labels else C.byref(labels), None)


def _label_sizes(n, K):
    return {"sort_expert_actions": K * n * 4, "press_expert_actions": K * n * 4, "stepped_actions": K * n * 4, "expert_stepped": K * n}


def test_labelled_rollout_memory():
    import torch

    from marl_sortingenv_amd._lib import MODULAR_BUFFER_NAMES, MODULAR_LABEL_BUFFER_NAMES

    n, K = 97, 4
    sort_ag, press_ag = _pair()
    env = _env(n, 0.05, base_seed=9)
    rng_before = env.get_state()[2].clone()
    raw, at = guarded(_sizes(n, K))
    lraw, lat = guarded(_label_sizes(n, K))
    ptrs = {name: raw.data_ptr() + off for name, (off, _) in at.items()}
    lptrs = {name: lraw.data_ptr() + off for name, (off, _) in lat.items()}
    # K - 1 steps into buffers of K rows: the last row of every [K, N, ...] buffer stays untouched, like the guards
    per_env = ("sort_last_values", "press_last_values", "last_dones")
    assert _raw_call(env, sort_ag, press_ag, K - 1, 64, ptrs, lptrs) == 0
    torch.cuda.synchronize()
    short = inside(raw, at, lambda name, size: size if name in per_env else size // K * (K - 1))
    lshort = inside(lraw, lat, lambda name, size: size // K * (K - 1))
    assert bool((raw[~short] == 0xA5).all()) and bool((lraw[~lshort] == 0xA5).all()), "a byte past the first K - 1 rows was written"
    assert _raw_call(env, sort_ag, press_ag, K, 64, ptrs, lptrs) == 0
    torch.cuda.synchronize()
    within, lwithin = inside(raw, at), inside(lraw, lat)
    assert bool((raw[~within] == 0xA5).all()) and bool((lraw[~lwithin] == 0xA5).all()), "a guard byte was written"
    # rng_sorting (words 18-23) and rng_pressing (words 12-17) are not touched, whoever steps
    assert torch.equal(rng_before[:, 12:24], env.get_state()[2][:, 12:24])
    # every output NULL, then one at a time with the others as they were
    assert _raw_call(env, sort_ag, press_ag, K, 64, {}, {}) == 0
    torch.cuda.synchronize()
    calls = 3
    for names, own, other, r in ((MODULAR_BUFFER_NAMES, ptrs, lptrs, raw), (MODULAR_LABEL_BUFFER_NAMES, lptrs, ptrs, lraw)):
        for name in names:
            before, lbefore = raw.clone(), lraw.clone()
            one = {name: own[name]}
            args = (one, {}) if own is ptrs else ({}, one)
            assert _raw_call(env, sort_ag, press_ag, 1, 64, *args) == 0, name
            torch.cuda.synchronize()
            calls += 1
            off, size = (at if own is ptrs else lat)[name]
            keep = torch.ones(r.numel(), dtype=torch.bool, device=r.device)
            keep[off:off + size] = False
            assert torch.equal(r[keep], (before if own is ptrs else lbefore)[keep]), f"{name}: another buffer changed"
            assert torch.equal(lraw if own is ptrs else raw, lbefore if own is ptrs else before), f"{name}: the other struct changed"
    assert torch.equal(rng_before[:, 12:24], env.get_state()[2][:, 12:24])
    assert env.policy_step == (K - 1) + K + K + (calls - 3) and env.error_count() == 0
    env.close()


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------
def _check_call(env, sort_ag, press_ag, K, flags=0, sort_seed=SORT_SEED, press_seed=PRESS_SEED, mix_seed=MIX_SEED, threshold=1 << 23):
    return env.L.mse_rollout_modular_labelled_check(None if env is None else env._h, None if sort_ag is None else sort_ag._h,
                                                    None if press_ag is None else press_ag._h, K, sort_seed, press_seed, mix_seed,
                                                    threshold, flags)


def test_labelled_rollout_refusals():
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
        lraw, lat = guarded(_label_sizes(n, K))
        ptrs = {name: raw.data_ptr() + off for name, (off, _) in at.items()}
        lptrs = {name: lraw.data_ptr() + off for name, (off, _) in lat.items()}
        assert _check_call(env, sort_ag, press_ag, K) == 0 and env.policy_step == 0  # the check launches nothing
        assert _raw_call(env, sort_ag, press_ag, K, 0, ptrs, lptrs) == 0
        torch.cuda.synchronize()
        filled, lfilled, state, t = raw.clone(), lraw.clone(), [x.clone() for x in env.get_state()], env.policy_step
        OUT_ONLY = ("struct_size", "label_struct_size", "no_out", "no_labels")

        def refused(status, e=env, s=sort_ag, p=press_ag, k=K, flags=0, message=None, **kw):
            """The check-only entry first: only a call it refuses is sent to the entry that could launch."""
            if not any(key in kw for key in OUT_ONLY):
                assert _check_call(e, s, p, k, flags, **kw) == status
            before = e.policy_step
            assert _raw_call(e, s, p, k, flags, ptrs, lptrs, **kw) == status
            if message is not None:
                assert message in e.L.mse_last_error(), e.L.mse_last_error()
            torch.cuda.synchronize()
            assert torch.equal(raw, filled) and torch.equal(lraw, lfilled), "a refused call wrote to the buffers"
            assert e.policy_step == before

        # 1. mse_rollout_modular's refusals, in its order
        refused(INVALID, s=None)
        refused(INVALID, p=None)
        press_env = keep(M.BatchedSortingEnv(kind="press", num_envs=n, device=0))
        refused(INVALID, e=press_env)
        refused(NOT_RESET, e=keep(_env(n, 0.05, reset_now=False)))
        refused(INVALID, k=0)
        no_reset = keep(_env(n, 0.05, auto_reset=False))
        refused(INVALID, e=no_reset)
        env.trace_begin(0, 16)
        refused(INVALID, message=b"trace")
        env.trace_end()
        for flag in (1, 4, 8, 16, 32, 512, 1 << 31):
            refused(INVALID, flags=flag, message=b"unknown rollout flag")
        refused(INVALID, s=press_ag)
        refused(INVALID, p=sort_ag)
        refused(INVALID, sort_seed=7, press_seed=7, message=b"sort_seed == press_seed")
        refused(UNSUPPORTED, s=M.MlpPolicy.random_init(13, 2, seed=1, precision="f32"))
        refused(UNSUPPORTED, e=keep(_env(n, 0.05, literal_choice=True)))
        gen_env = keep(_env(n, 0.05, config=replay.sorting_config(GEN_META)))
        refused(UNSUPPORTED, e=gen_env)
        # tables that do not fit: served in 32-env waves, refused in 64-env waves, as in the plain kernel
        big_cfg = replay.sorting_config(BIG_TABLES_META)
        small_big = keep(_env(n, 0.05, config=big_cfg))
        assert _check_call(small_big, sort_ag, press_ag, K) == 0
        big = keep(_env(256 * cus() + 1, 0.05, config=big_cfg))
        refused(UNSUPPORTED, e=big, message=b"LDS image does not fit")
        # an earlier refusal wins over a later one: the plain kernel's before the threshold's, the threshold's before the seed's
        refused(INVALID, k=0, threshold=ONE + 1, message=b"k_steps")
        # 2. the threshold
        refused(INVALID, threshold=ONE + 1, message=b"expert_threshold")
        refused(INVALID, threshold=ONE + 1, mix_seed=SORT_SEED, message=b"expert_threshold")
        refused(INVALID, threshold=0xFFFFFFFF, message=b"expert_threshold")
        # 3. the mixture seed, whatever the threshold
        for thr in (0, 1 << 23, ONE):
            refused(INVALID, mix_seed=SORT_SEED, threshold=thr, message=b"mix_seed")
            refused(INVALID, mix_seed=PRESS_SEED, threshold=thr, message=b"mix_seed")
        refused(INVALID, mix_seed=SORT_SEED, no_out=True, message=b"mix_seed")
        # 4. the structs
        refused(INVALID, no_out=True, message=b"out is NULL")
        refused(INVALID, struct_size=8, message=b"mse_modular_buffers")
        refused(INVALID, no_labels=True, message=b"labels is NULL")
        refused(INVALID, label_struct_size=8, message=b"mse_modular_label_buffers")
        refused(INVALID, no_out=True, no_labels=True, message=b"out is NULL")
        assert _check_call(env, sort_ag, press_ag, K, threshold=0) == 0 and _check_call(env, sort_ag, press_ag, K, threshold=ONE) == 0
        for x, y in zip(state, env.get_state()):
            assert torch.equal(x, y)
        assert env.policy_step == t
        # Python refuses the same, both classes
        for cls in (M.FusedModularRollout, M.ModularRolloutCollector):
            for bad in (dict(mix_seed=SORT_SEED), dict(mix_seed=PRESS_SEED), dict(beta=1.5), dict(beta=-0.1), dict(beta=float("nan"))):
                with pytest.raises(ValueError):
                    cls(env, sort_ag, press_ag, K, SORT_SEED, PRESS_SEED, expert_labels=True, **bad)
            for bad in (dict(beta=0.5), dict(mix_seed=MIX_SEED), dict(gamma=0.99)):
                with pytest.raises(ValueError):
                    cls(env, sort_ag, press_ag, K, SORT_SEED, PRESS_SEED, **bad)
            plain = cls(env, sort_ag, press_ag, K, SORT_SEED, PRESS_SEED)
            with pytest.raises(ValueError, match="demo_view"):
                plain.demo_view("sort")
            with pytest.raises(ValueError):
                plain.beta = 0.5
            assert plain.beta == 0.0 and "expert_actions" not in plain.view("sort", "team") and "mix_seed" not in plain.state_dict()
            lab = cls(env, sort_ag, press_ag, K, SORT_SEED, PRESS_SEED, expert_labels=True)
            assert lab.mix_seed not in (SORT_SEED, PRESS_SEED) and lab.beta == 0.0
            with pytest.raises(ValueError):
                lab.beta = 2.0
            assert lab.beta == 0.0
            lab.beta = 1.0
            assert lab.view("press", "team")["expert_actions"] is lab.buffers["press_expert_actions"]
            assert lab.demo_view("sort")["returns"] is None
            sd = lab.state_dict()
            assert sd["mix_seed"] == lab.mix_seed and sd["beta"] == 1.0
            with pytest.raises(ValueError):
                plain.check_state_dict(sd)
            with pytest.raises(ValueError):
                lab.check_state_dict(plain.state_dict())
            with pytest.raises(M.MseError) as err:
                cls(big, sort_ag, press_ag, K, SORT_SEED, PRESS_SEED, expert_labels=True).collect()
            assert err.value.status == UNSUPPORTED
        assert env.policy_step == t and big.policy_step == 0
    finally:
        for e in opened:
            e.close()
