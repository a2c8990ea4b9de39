"""GPU: the lookahead kernel (`mse_lookahead`, `BatchedSortingEnv.lookahead`) - against its multi-launch twin
`lookahead_reference` bit for bit, with own streams against the real env stepped by the existing calls, at an exact tie,
for what it must leave untouched, in every refusal in the header's order - and `LookaheadCollector` /
`evaluate_lookahead` against hand loops over the same calls.

Common setup: N = 300 envs (one full workgroup of 256 and a partial one), max_steps = 20, warmed with 15 masked-random
steps: presses are busy, the masks differ between envs, and at H = 9 every fork runs into its episode's end after 5 steps."""
import ctypes as C

import pytest

from tests.rollout_checks import bits_equal

pytestmark = pytest.mark.gpu

N, MAX_STEPS, WARM = 300, 20, 15
INVALID, UNSUPPORTED, NOT_RESET, ALIGNMENT = -1, -2, -5, -6
KEYS = ("q", "action", "value")


def _env(kind, noise, max_steps=MAX_STEPS, n=N, warm=WARM, **kw):
    import marl_sortingenv_amd as M

    env = M.BatchedSortingEnv(kind=kind, num_envs=n, base_seed=31, max_steps=max_steps, noise_sorting=noise,
                              balesize=kw.pop("balesize", 200), **kw)
    for _ in range(warm):
        env.step(env.sample_actions(7))
    return env


def _state_bits(env):
    import torch

    return [t.clone() for t in env.get_state()] + [env.obs.clone().view(torch.int32), env.mask.clone()]


def _same_state(before, env):
    import torch

    return all(torch.equal(a, b) for a, b in zip(before, _state_bits(env)))


def _check_inputs(env):
    """The inputs have what the cases need: a forbidden candidate, an env with >= 3 legal ones (where the kind has masks),
    and WARM steps behind every env, so that a fork of 9 steps ends after MAX_STEPS - WARM = 5."""
    mask = env.action_masks()
    if env.kind == "sort":
        assert bool((mask == 1).all())
    else:
        assert bool((mask == 0).any()), "no forbidden candidate"
        assert bool((mask.sum(dim=1) >= 3).any()), "no env with three legal candidates"
        assert mask.unique(dim=0).shape[0] > 1, "the masks do not differ between envs"
    assert bool((env.get_state()[0][:, 32] == WARM).all())


# every value of every axis (noise, H, gamma, streams, base policy, M) at least once per kind
CASES = [(0.0, 1, 1.0, "own", "rule_based", 1),
         (0.05, 2, 0.9, "fresh", "random", 3),
         (0.05, 9, 0.9, "own", "random", 1),
         (0.0, 9, 1.0, "fresh", "rule_based", 3)]


def _compare(env, tag, **kw):
    import torch

    import marl_sortingenv_amd as M

    got = env.lookahead(**kw)
    exp = M.lookahead_reference(env, **kw)
    torch.cuda.synchronize()
    assert set(got) == set(KEYS) == set(exp)
    legal = env.action_masks().t().ne(0)
    assert torch.equal(torch.isneginf(got["q"]), ~legal), tag  # the -inf pattern is the mask's
    assert bool(torch.isfinite(got["q"][legal]).all()) and bool(torch.isfinite(got["value"]).all())
    print(f"{tag}: q in [{float(got['q'][legal].min()):.6f}, {float(got['q'][legal].max()):.6f}], "
          f"{int((got['q'] != exp['q']).sum())} q cells / {int((got['action'] != exp['action']).sum())} actions differ")
    bits_equal(tag, {k: got[k].view(torch.int64) if got[k].dtype == torch.float64 else got[k] for k in KEYS},
               {k: exp[k].view(torch.int64) if exp[k].dtype == torch.float64 else exp[k] for k in KEYS}, KEYS)
    return got


@pytest.mark.parametrize("kind", ["sort", "press", "mono"])
@pytest.mark.parametrize("noise, horizon, gamma, streams, base, m", CASES,
                         ids=[f"noise{c[0]}-H{c[1]}-g{c[2]}-{c[3]}-{c[4]}-M{c[5]}" for c in CASES])
def test_kernel_equals_reference(kind, noise, horizon, gamma, streams, base, m):
    env = _env(kind, noise)
    _check_inputs(env)
    before = _state_bits(env)
    got = _compare(env, f"{kind}", horizon=horizon, gamma=gamma, base_policy=base, streams=streams, seed=5, base_seed=77,
                   n_samples=m)
    assert _same_state(before, env)
    if kind != "sort":  # the chosen action is legal and its q is the column's maximum
        import torch

        mask = env.action_masks()
        assert bool(mask.gather(1, got["action"].long().view(-1, 1)).ne(0).all())
        assert torch.equal(got["value"], got["q"].max(dim=0).values)


def test_every_fork_ends_early_at_h9():
    """H = 9 and H = 5 give the same bits when 5 steps are left: steps after `done` add nothing (no auto-reset in a fork)."""
    import torch

    env = _env("mono", 0.0)
    _check_inputs(env)
    a, b = env.lookahead(9, streams="own"), env.lookahead(MAX_STEPS - WARM, streams="own")
    c = env.lookahead(MAX_STEPS - WARM - 1, streams="own")
    assert torch.equal(a["q"].view(torch.int64), b["q"].view(torch.int64)) and torch.equal(a["action"], b["action"])
    assert not torch.equal(a["q"].view(torch.int64), c["q"].view(torch.int64))


def test_press_with_sort_mode_tensor():
    import torch

    env = _env("press", 0.05)
    _check_inputs(env)
    sm = (torch.arange(N, device="cuda") % 2).to(torch.int32)
    with_sm = _compare(env, "press sort_mode", horizon=4, gamma=0.9, streams="fresh", seed=3, n_samples=2, sort_mode=sm)
    without = env.lookahead(4, gamma=0.9, streams="fresh", seed=3, n_samples=2)
    assert not torch.equal(with_sm["q"].view(torch.int64), without["q"].view(torch.int64))  # the tensor is read


def test_check_overflow_fires():
    """A small balesize (the random warm-up presses early and keeps both presses busy) and containers of 500 units: within
    three steps some forks overflow - the -10 penalty, then nothing - and others do not."""
    import torch

    from marl_sortingenv_amd.config import SortingEnvConfig

    cfg = SortingEnvConfig().with_overrides({"pressing_station": {"container_capacity": 500}})
    env = _env("mono", 0.0, balesize=50, config=cfg)
    pen = float(cfg.overflow_termination_penalty)
    got = _compare(env, "mono overflow", horizon=3, gamma=1.0, streams="own", check_overflow=True)
    off = env.lookahead(3, gamma=1.0, streams="own")
    legal = env.action_masks().t().ne(0)
    fired = (got["q"] != off["q"]) & legal  # the penalty replaced a reward, or ended the fork
    first = (got["q"] == pen) & legal
    print(f"overflow: of {int(legal.sum())} legal forks {int(fired.sum())} overflow within 3 steps, {int(first.sum())} on their first")
    assert bool(fired.any()) and bool((~fired & legal).any())
    assert bool((got["q"][fired] < off["q"][fired]).all())


@pytest.mark.parametrize("kind, noise", [("mono", 0.0), ("mono", 0.05), ("press", 0.05), ("sort", 0.05)])
def test_own_streams_equal_real_stepping(kind, noise):
    """Independent of the twin: take `action`, step the REAL env with it, then 8 rule-based steps through the existing
    calls, and sum reward64 by the header's rule: the sum is `value`, bit for bit, for every env."""
    import torch

    H, gamma = 9, 0.9
    env = _env(kind, noise, max_steps=200)
    la = env.lookahead(H, gamma=gamma, base_policy="rule_based", streams="own")
    action, value = la["action"].clone(), la["value"].clone()
    acc = torch.zeros(N, dtype=torch.float64, device="cuda")
    disc = 1.0
    for s in range(H):
        env.step(action if s == 0 else env.rule_actions(), want_reward64=True)
        assert not bool(env.done.any())
        acc = acc + disc * env.reward64
        disc = disc * gamma
    torch.cuda.synchronize()
    print(f"{kind} noise {noise}: value in [{float(value.min()):.6f}, {float(value.max()):.6f}], "
          f"{int((acc != value).sum())} of {N} differ from real stepping")
    assert torch.equal(acc.view(torch.int64), value.view(torch.int64))


def test_ties_go_to_the_lowest_index():
    """Right after reset on mono at H = 1 candidates 0 and 11 (sensor mode 0 / 1, no press) are both legal and tie exactly:
    the first step sorts nothing."""
    import torch

    env = _env("mono", 0.0, warm=0)
    for streams in ("own", "fresh"):
        la = env.lookahead(1, streams=streams)
        mask = env.action_masks()
        assert bool(mask[:, 0].all()) and bool(mask[:, 11].all())
        assert bool((la["q"][0] == la["q"][11]).all())
        assert bool((la["action"] == 0).all())
        assert torch.equal(la["value"].view(torch.int64), la["q"][0].view(torch.int64))


def _raw(env, horizon=3, gamma=1.0, base=1, base_seed=2024, streams=1, seed=0, m=1, sort_mode=None, flags=0, q=None, action=None,
         value=None, ws=None, h="env"):
    import torch

    p = lambda t: None if t is None else C.c_void_p(t if isinstance(t, int) else t.data_ptr())  # noqa: E731
    return env.L.mse_lookahead(env._h if h == "env" else h, horizon, gamma, base, base_seed, streams, seed, m, p(sort_mode), flags,
                               p(q), p(action), p(value), p(ws), C.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_nothing_else_is_touched():
    import torch

    GUARD, M_S = 64, 3
    env, twin = _env("mono", 0.05), _env("mono", 0.05)
    A = env.num_actions
    sizes = {"q": 8 * A * N, "action": 4 * N, "value": 8 * N, "ws": int(env.L.mse_lookahead_workspace_bytes(env._h, M_S))}
    assert sizes["ws"] == 8 * M_S * A * N

    def buffers():
        raw, at, off = None, {}, GUARD
        for name, size in sizes.items():
            at[name] = (off, size)
            off += (size + 15) // 16 * 16 + GUARD
        raw = torch.full((off,), 0xA5, dtype=torch.uint8, device="cuda")
        return raw, at

    def inside(raw, at, names):
        m = torch.zeros(raw.numel(), dtype=torch.bool, device="cuda")
        for name in names:
            m[at[name][0]:at[name][0] + at[name][1]] = True
        return m

    before, t0, errors = _state_bits(env), env.policy_step, env.error_count()
    raw, at = buffers()
    ptr = {k: raw.data_ptr() + at[k][0] for k in at}
    kw = dict(horizon=4, gamma=0.9, base=0, base_seed=9, streams=1, seed=11, m=M_S)
    assert _raw(env, q=ptr["q"], action=ptr["action"], value=ptr["value"], ws=ptr["ws"], **kw) == 0
    torch.cuda.synchronize()
    assert bool((raw[~inside(raw, at, at)] == 0xA5).all()), "a guard byte was written"
    assert _same_state(before, env) and env.policy_step == t0 and env.error_count() == errors
    # action_out = value_out = NULL: q is the same, the two are not written
    raw2, at2 = buffers()
    ptr2 = {k: raw2.data_ptr() + at2[k][0] for k in at2}
    assert _raw(env, q=ptr2["q"], ws=ptr2["ws"], **kw) == 0
    torch.cuda.synchronize()
    assert bool((raw2[~inside(raw2, at2, ("q", "ws"))] == 0xA5).all())
    assert torch.equal(raw2[inside(raw2, at2, ("q",))], raw[inside(raw, at, ("q",))])
    # a rerun gives equal bits
    raw3, at3 = buffers()
    ptr3 = {k: raw3.data_ptr() + at3[k][0] for k in at3}
    assert _raw(env, q=ptr3["q"], action=ptr3["action"], value=ptr3["value"], ws=ptr3["ws"], **kw) == 0
    torch.cuda.synchronize()
    assert torch.equal(raw3, raw)
    # and the method returns the same bits as the raw call
    la = env.lookahead(4, gamma=0.9, base_policy="random", base_seed=9, streams="fresh", seed=11, n_samples=M_S)
    q_raw = raw[at["q"][0]:at["q"][0] + at["q"][1]].view(torch.int64)
    assert torch.equal(la["q"].view(torch.int64).reshape(-1), q_raw)
    # a following rollout() gives the bits it gives without the lookahead call
    got, exp = env.rollout(6, policy_seed=3), twin.rollout(6, policy_seed=3)
    torch.cuda.synchronize()
    for key in got:
        assert torch.equal(got[key].view(torch.uint8), exp[key].view(torch.uint8)), key
    assert all(torch.equal(a, b) for a, b in zip(env.get_state(), twin.get_state()))


def test_refusals_in_the_headers_order():
    import torch

    import marl_sortingenv_amd as M

    env = _env("mono", 0.0, n=64, warm=2)
    press = _env("press", 0.0, n=64, warm=2)
    A = env.num_actions
    q = torch.full((A * 64 + 1,), 7.0, dtype=torch.float64, device="cuda")
    ws = torch.full((A * 64 + 1,), 7.0, dtype=torch.float64, device="cuda")
    val = torch.full((65,), 7.0, dtype=torch.float64, device="cuda")
    act = torch.full((64,), 7, dtype=torch.int32, device="cuda")
    sm = torch.zeros(64, dtype=torch.int32, device="cuda")
    ok = dict(q=q, action=act, value=val, ws=ws)
    L = env.L
    odd = lambda t: t.data_ptr() + 4  # noqa: E731  4 mod 8

    def refused(status, word, e=env, **kw):
        assert _raw(e, **dict(ok, **kw)) == status, (word, L.mse_last_error())
        assert word.encode() in L.mse_last_error(), (word, L.mse_last_error())

    # each call is wrong in what it names AND in everything the header lists after it: the earlier refusal wins
    later = dict(horizon=0, m=0, gamma=2.0, base=2, flags=1, sort_mode=sm, q=odd(q))
    refused(INVALID, "NULL", h=None, **later)
    refused(INVALID, "NULL", **dict(later, q=None))
    refused(INVALID, "NULL", **dict(later, ws=None))
    refused(INVALID, "horizon", **later)
    refused(INVALID, "horizon", **dict(later, horizon=65536))
    later.pop("horizon")
    refused(INVALID, "n_samples", **later)
    refused(INVALID, "n_samples", **dict(later, m=257))
    later.pop("m")
    for g in (2.0, -0.1, float("nan"), float("inf")):
        refused(INVALID, "gamma", **dict(later, gamma=g))
    later.pop("gamma")
    refused(INVALID, "base_policy", **later)
    refused(INVALID, "base_policy", **dict(later, base=-1))
    refused(INVALID, "streams", **dict(later, base=1, streams=2))
    later.pop("base")
    for f in (1, 4, 8, 2 | 4):  # MSE_STEP_UNMASKED, MSE_ROLLOUT_RULE_BASED, MSE_STEP_SANITIZE_LATE
        refused(INVALID, "MSE_STEP_CHECK_OVERFLOW", **dict(later, flags=f))
    later.pop("flags")
    refused(INVALID, "sort_mode_dev", **later)
    later.pop("sort_mode")
    refused(ALIGNMENT, "8-byte", **later)
    refused(ALIGNMENT, "8-byte", value=odd(val))
    refused(ALIGNMENT, "8-byte", ws=odd(ws))
    # general generator mode, by name; a handle not yet reset; both before the alignment
    from marl_sortingenv_amd.config import SortingEnvConfig

    gen = M.BatchedSortingEnv("mono", num_envs=64, max_steps=MAX_STEPS, noise_sorting=0.0,
                              config=SortingEnvConfig().with_overrides({"simulation": {"input_batch_size": 90}}))
    refused(UNSUPPORTED, "general generator mode", e=gen, q=odd(q))
    cold = M.BatchedSortingEnv("mono", num_envs=64, max_steps=MAX_STEPS, noise_sorting=0.0, reset_now=False)
    refused(NOT_RESET, "mse_reset", e=cold, q=odd(q))
    torch.cuda.synchronize()
    assert bool((q == 7.0).all()) and bool((ws == 7.0).all()) and bool((val == 7.0).all()) and bool((act == 7).all())
    # the accepted forms next to them
    assert _raw(press, sort_mode=sm, q=q, ws=ws, flags=2) == 0
    assert _raw(env, horizon=1, gamma=0.0, m=1, **ok) == 0 and _raw(env, gamma=1.0, base=0, streams=0, **ok) == 0
    assert int(L.mse_lookahead_workspace_bytes(env._h, 0)) == INVALID and int(L.mse_lookahead_workspace_bytes(env._h, 257)) == INVALID
    assert int(L.mse_lookahead_workspace_bytes(env._h, 256)) == 8 * 256 * A * 64
    with pytest.raises(M.MseError):
        gen.lookahead(2)


def _actor(kind, seed=3):
    from tests.test_gpu_demo_rollout import _actor as demo_actor  # an untrained student whose draws and argmax matter

    return demo_actor(kind, seed=seed)


@pytest.mark.parametrize("with_actor", [False, True], ids=["planner-steps", "student-steps"])
def test_collector_equals_its_docstrings_loop(with_actor):
    import torch

    import marl_sortingenv_amd as M
    from marl_sortingenv_amd.learner import _ptr, _stream

    K, H, GAMMA, SEED = 7, 3, 0.95, 40
    kw = dict(base_policy="random", streams="fresh", base_seed=12, n_samples=2)
    a, b = _env("mono", 0.05, max_steps=5, warm=0), _env("mono", 0.05, max_steps=5, warm=0)
    actor = _actor("mono") if with_actor else None
    col = M.LookaheadCollector(a, K, H, actor=actor, gamma=GAMMA, seed=SEED, **kw)
    got = col.collect()
    # the hand loop
    n, dev = N, "cuda"
    exp = {"observations": torch.empty((K, n, 29), device=dev), "action_masks": torch.empty((K, n, 22), dtype=torch.uint8, device=dev),
           "episode_starts": torch.empty((K, n), dtype=torch.uint8, device=dev), "rewards": torch.empty((K, n), device=dev),
           "returns": torch.empty((K, n), device=dev), "values": torch.empty((K, n), dtype=torch.float64, device=dev),
           **{k: torch.empty((K, n), dtype=torch.int32, device=dev) for k in ("actions", "rule_actions", "stepped_actions")}}
    last = torch.ones(n, dtype=torch.uint8, device=dev)  # the envs were just reset
    for k in range(K):
        la = b.lookahead(H, gamma=GAMMA, seed=SEED + k, **kw)
        exp["observations"][k], exp["action_masks"][k], exp["episode_starts"][k] = b.obs, b.mask, last
        exp["actions"][k], exp["values"][k], exp["rule_actions"][k] = la["action"], la["value"], b.rule_actions()
        stepped = la["action"] if actor is None else \
            actor.forward(b.obs, b.mask, seed=SEED, t=k, deterministic=False, index_offset=b.index_offset)["action"]
        exp["stepped_actions"][k] = stepped
        _, rew, done, _ = b.step(exp["stepped_actions"][k])
        exp["rewards"][k] = rew
        last = done.clone()
    exp["last_dones"] = last
    zeros, adv = torch.zeros((K + 1, n), device=dev), torch.empty((K, n), device=dev)
    assert b.L.mse_gae(K, n, _ptr(exp["rewards"]), _ptr(zeros), _ptr(exp["episode_starts"]), _ptr(zeros[K]), _ptr(last), GAMMA, 1.0,
                       _ptr(adv), _ptr(exp["returns"]), _stream(b.device)) == 0
    torch.cuda.synchronize()
    assert set(got) == set(exp)
    view = lambda d: {k: (v.view(torch.int64) if v.dtype == torch.float64 else v) for k, v in d.items()}  # noqa: E731
    bits_equal("collector", view(got), view(exp), sorted(exp))
    assert all(torch.equal(x, y) for x, y in zip(a.get_state(), b.get_state())) and a.policy_step == b.policy_step
    assert bool(got["episode_starts"].any()) and bool((got["actions"] != got["rule_actions"]).any())
    if with_actor:
        assert bool((got["stepped_actions"] != got["actions"]).any())
    else:
        assert torch.equal(got["stepped_actions"], got["actions"])
    # one ImitationLearner.update() on the dict
    student = _actor("mono", seed=9)
    stats = M.ImitationLearner(student, batch_size=512, seed=1).update(got)["mean"]
    print("update:", stats)
    assert all(v == v and abs(v) != float("inf") for k, v in stats.items() if k != "_") and stats["unusable"] == 0


def test_evaluate_lookahead_equals_hand_loop():
    import torch

    import marl_sortingenv_amd as M
    from marl_sortingenv_amd.episodes import eval_targets

    n, max_steps, H, episodes = 10, 30, 4, 25
    kw = dict(streams="fresh", n_samples=2, seed=6, gamma=0.9)
    a = M.BatchedSortingEnv("mono", num_envs=n, base_seed=100, max_steps=max_steps, noise_sorting=0.0)
    b = M.BatchedSortingEnv("mono", num_envs=n, base_seed=100, max_steps=max_steps, noise_sorting=0.0)
    mean, std = M.evaluate_lookahead(a, episodes, H, **kw)
    # the hand loop: SB3's counting rule through EpisodeStats
    b.reset(seeds=b.seeds)
    b.policy_step = 0
    targets = eval_targets(episodes, n)
    stats = M.EpisodeStats(n, b.device, slots=max(targets), targets=targets)
    buf = {"reward": torch.empty((max_steps, n), device="cuda"), "done": torch.empty((max_steps, n), dtype=torch.uint8, device="cuda")}
    t = 0
    for _ in range(max(targets)):
        for k in range(max_steps):
            la = b.lookahead(H, streams="fresh", n_samples=2, seed=6 + t, gamma=0.9)
            _, rew, done, _ = b.step(la["action"])
            buf["reward"][k], buf["done"][k] = rew, done
            t += 1
        stats.update(buf)
    s = stats.summary()
    print(f"evaluate_lookahead: {mean} +- {std} over {s['episodes']} episodes")
    assert s["episodes"] == episodes
    assert mean == s["mean_return"] and std == s["std_return"]
    assert all(torch.equal(x, y) for x, y in zip(a.get_state(), b.get_state()))
