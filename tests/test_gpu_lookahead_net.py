"""GPU: the lookahead with a network inside the fork (`mse_lookahead_net`: an `MlpPolicy` as `base_policy` and / or
`leaf_value` of `BatchedSortingEnv.lookahead`) - against its multi-launch twin `lookahead_reference` bit for bit, over what
the horizons cover, with desynchronised lanes in one wave, at H = 1 against a hand loop over existing calls, for what it must
leave untouched, for when the weights are read, in every refusal in the header's order - and `LookaheadCollector` /
`evaluate_lookahead` with a network against hand loops.

Every comparison is on bits (q viewed as int64): the fused forward equals `mse_policy_forward` on bits
(tests/test_gpu_policy.py) and the returns are formed with separately rounded operations, so no tolerance is needed.

Setup as tests/test_gpu_lookahead.py: N = 300 envs (a full workgroup and a partial one whose last wave is partial),
max_steps = 20, 15 masked-random warm-up steps (5 steps left in every episode), an untrained network of the env's shape."""
import ctypes as C

import pytest

from tests.rollout_checks import bits_equal
from tests.test_gpu_lookahead import KEYS, MAX_STEPS, N, WARM, _check_inputs, _env, _same_state, _state_bits

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED, NOT_RESET, ALIGNMENT = -1, -2, -5, -6
LEFT = MAX_STEPS - WARM  # steps left in every episode


def _policy(kind, precision="f16x3", seed=3):
    from tests.test_gpu_demo_rollout import _actor  # random_init of the env's shape, the action head scaled so that argmax and draws matter

    return _actor(kind, precision=precision, seed=seed)


def _bits(d):
    import torch

    return {k: d[k].view(torch.int64) if d[k].dtype == torch.float64 else d[k] for k in KEYS}


def _same_bits(a, b):
    import torch

    return all(torch.equal(x, y) for x, y in zip(_bits(a).values(), _bits(b).values()))


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
    bits_equal(tag, _bits(got), _bits(exp), KEYS)
    return got


def _network_kw(p, base, leaf):
    """base: "argmax" | "sampled" (the network) or one of mse_lookahead's strings."""
    kw = dict(base_policy=p if base in ("argmax", "sampled") else base, leaf_value=p if leaf else None)
    if base in ("argmax", "sampled"):
        kw["base_deterministic"] = base == "argmax"
    return kw


# every value of every axis (noise, precision, base, leaf, H, gamma, streams, M) at least once per kind
CASES = [(0.0, "f32", "argmax", False, 2, 1.0, "own", 1),
         (0.05, "f16x3", "sampled", True, 4, 0.9, "fresh", 3),
         (0.0, "f16x3", "rule_based", True, 1, 0.9, "fresh", 1),
         (0.05, "f32", "random", True, 5, 1.0, "own", 3),
         (0.05, "f32", "sampled", False, 9, 0.9, "fresh", 1),
         (0.0, "f16x3", "argmax", True, 9, 1.0, "own", 1)]


def test_case_list_covers_every_axis():
    axes = list(zip(*CASES))
    want = [{0.0, 0.05}, {"f32", "f16x3"}, {"argmax", "sampled", "rule_based", "random"}, {True, False}, {1, 2, 4, 5, 9}, {1.0, 0.9},
            {"own", "fresh"}, {1, 3}]
    assert [set(a) for a in axes] == want
    assert all(leaf for _, _, base, leaf, *_ in CASES if base in ("rule_based", "random"))


@pytest.mark.parametrize("kind", ["sort", "press", "mono"])
@pytest.mark.parametrize("noise, precision, base, leaf, horizon, gamma, streams, m", CASES,
                         ids=[f"noise{c[0]}-{c[1]}-{c[2]}-leaf{int(c[3])}-H{c[4]}-g{c[5]}-{c[6]}-M{c[7]}" for c in CASES])
def test_kernel_equals_reference(kind, noise, precision, base, leaf, horizon, gamma, streams, m):
    import torch

    env = _env(kind, noise)
    _check_inputs(env)  # a forbidden candidate and an env with >= 3 legal ones (press, mono); WARM steps behind every env
    p = _policy(kind, precision)
    assert p.precision == precision
    before = _state_bits(env)
    got = _compare(env, f"{kind}", horizon=horizon, gamma=gamma, streams=streams, seed=5, base_seed=77, n_samples=m,
                   **_network_kw(p, base, leaf))
    assert _same_state(before, env)
    if kind != "sort":  # the chosen action is legal and its q is the column's maximum
        mask = env.action_masks()
        assert bool(mask.gather(1, got["action"].long().view(-1, 1)).ne(0).all())
        assert torch.equal(got["value"], got["q"].max(dim=0).values)


@pytest.mark.parametrize("kind", ["press", "mono"])
def test_the_network_base_is_used_and_its_draws_matter(kind):
    """Checks on the inputs of the cases above: the network base changes q against the rule's, and the sampled base differs
    from the argmax base."""
    import torch

    env, p = _env(kind, 0.05), _policy(kind)
    kw = dict(horizon=4, gamma=0.9, streams="fresh", seed=5, base_seed=77)
    rule = env.lookahead(base_policy="rule_based", **kw)
    argmax = env.lookahead(base_policy=p, **kw)
    sampled = env.lookahead(base_policy=p, base_deterministic=False, **kw)
    other_draws = env.lookahead(base_policy=p, base_deterministic=False, **dict(kw, base_seed=78))
    torch.cuda.synchronize()
    legal = env.action_masks().t().ne(0)
    for name, a, b in (("rule / argmax", rule, argmax), ("argmax / sampled", argmax, sampled), ("base_seed 77 / 78", sampled, other_draws)):
        differ = int(((a["q"] != b["q"]) & legal).sum())
        print(f"{kind} {name}: {differ} of {int(legal.sum())} legal cells differ")
        assert differ > 0, name
    # base_deterministic is ignored for the string bases
    leaf = dict(kw, base_policy="rule_based", leaf_value=p)
    assert _same_bits(env.lookahead(base_deterministic=True, **leaf), env.lookahead(base_deterministic=False, **leaf))


@pytest.mark.parametrize("base", ["argmax", "rule_based"])
def test_what_the_horizons_cover(base):
    """5 steps are left in every episode.  H = 4: every legal fork bootstraps.  H = 5 ends on its last step: no fork
    bootstraps, it equals H = 9 on bits, and the leaf changes nothing there.  H = 2 with the leaf differs from H = 2 without."""
    import torch

    env, p = _env("mono", 0.0), _policy("mono")
    _check_inputs(env)
    legal = env.action_masks().t().ne(0)
    kw = dict(gamma=0.9, streams="own")
    base_kw = dict(base_policy=p, base_deterministic=True) if base == "argmax" else dict(base_policy=base)

    def run(h, leaf):
        if not leaf and base != "argmax":  # no network in the call: mse_lookahead
            return {k: v.clone() for k, v in env.lookahead(h, **kw, **base_kw).items()}
        return {k: v.clone() for k, v in env.lookahead(h, leaf_value=p if leaf else None, **kw, **base_kw).items()}

    on4, off4 = _compare(env, f"{base} H4 leaf", horizon=LEFT - 1, leaf_value=p, **kw, **base_kw), run(LEFT - 1, False)
    changed = (on4["q"] != off4["q"])
    print(f"H = {LEFT - 1}: the leaf changes {int(changed[legal].sum())} of {int(legal.sum())} legal forks")
    assert bool(changed[legal].all()) and not bool(changed[~legal].any())
    on5, off5, on9, off9 = run(LEFT, True), run(LEFT, False), run(9, True), run(9, False)
    assert _same_bits(on5, off5) and _same_bits(on5, on9) and _same_bits(on9, off9)
    assert not _same_bits(on5, on4)
    on2, off2 = run(2, True), run(2, False)
    assert bool(((on2["q"] != off2["q"]) & legal).any()) and not _same_bits(on2, off2)
    # the leaf is gamma^H x value: at gamma = 0 it adds +-0 and leaves every q as it was
    zero_on = env.lookahead(2, gamma=0.0, streams="own", leaf_value=p, **base_kw)
    zero_off = env.lookahead(2, gamma=0.0, streams="own", **base_kw)
    assert torch.equal(zero_on["q"], zero_off["q"])


@pytest.mark.parametrize("kind, noise", [("mono", 0.05), ("press", 0.0)])
def test_desynchronised_lanes(kind, noise):
    """Two warmed handles, 13 and 17 steps behind them, spliced row by row (i % 2): at H = 5 with the leaf the odd lanes'
    forks end after 3 steps while their wave neighbours reach the leaf."""
    import torch

    early, late, env = _env(kind, noise, warm=13), _env(kind, noise, warm=17), _env(kind, noise, warm=0)
    odd = (torch.arange(N, device="cuda") % 2).bool().view(N, 1)
    env.set_state(*[torch.where(odd, b, a) for a, b in zip(early.get_state(), late.get_state())])
    steps = env.get_state()[0][:, 32]
    assert torch.equal(steps, torch.where(odd.view(N), 17, 13).to(steps.dtype))
    for w in range(0, N, 64):  # both groups in every wave
        assert set(steps[w:w + 64].tolist()) == {13, 17}
    p = _policy(kind)
    H = 5
    assert MAX_STEPS - 17 < H <= MAX_STEPS - 13
    for base in ("argmax", "sampled", "rule_based"):
        kw = dict(horizon=H, gamma=0.9, streams="fresh", seed=2, base_seed=8, n_samples=2, **_network_kw(p, base, True))
        on = _compare(env, f"{kind} spliced {base}", **kw)
        off = env.lookahead(**dict(kw, leaf_value=None)) if base != "rule_based" else \
            env.lookahead(horizon=H, gamma=0.9, streams="fresh", seed=2, base_seed=8, n_samples=2, base_policy="rule_based")
        legal = env.action_masks().t().ne(0)
        changed = on["q"] != off["q"]
        odd_cols = odd.view(1, N).expand_as(legal)
        assert bool(changed[legal & ~odd_cols].all()), "an even lane's fork did not reach the leaf"
        assert not bool(changed[odd_cols].any()), "an odd lane's fork added a leaf after its episode's end"
        assert bool((legal & odd_cols).any()) and bool((legal & ~odd_cols).any())


@pytest.mark.parametrize("kind, noise, precision", [("mono", 0.05, "f16x3"), ("press", 0.0, "f32"), ("sort", 0.05, "f32")])
def test_h1_with_leaf_equals_hand_loop(kind, noise, precision):
    """The TD-greedy reading, independent of the twin: per legal candidate, step a copy of the state (own streams) and add
    gamma x the critic's value of the observation the step returns."""
    import torch

    GAMMA = 0.9
    env, scratch, p = _env(kind, noise), _env(kind, noise, warm=0), _policy(kind, precision)
    la = env.lookahead(1, gamma=GAMMA, streams="own", leaf_value=p)
    state = env.get_state()
    mask = env.action_masks()
    first_legal = mask.ne(0).to(torch.int32).argmax(dim=1).to(torch.int32)
    q = torch.full((env.num_actions, N), float("-inf"), dtype=torch.float64, device="cuda")
    for a in range(env.num_actions):
        legal = mask[:, a].ne(0)
        scratch.set_state(*state)
        scratch.step(torch.where(legal, torch.full_like(first_legal, a), first_legal), want_reward64=True)
        assert not bool(scratch.done.any())
        value = p.forward(scratch.obs, scratch.mask, deterministic=True)["value"].double()
        q[a] = torch.where(legal, scratch.reward64 + GAMMA * value, q[a])
    torch.cuda.synchronize()
    print(f"{kind} {precision}: {int((q != la['q']).sum())} of {q.numel()} cells differ from the hand loop")
    assert torch.equal(q.view(torch.int64), la["q"].view(torch.int64))
    assert torch.equal(la["value"].view(torch.int64), q.max(dim=0).values.view(torch.int64))


def _raw(env, policy, horizon=3, gamma=1.0, base=2, det=1, base_seed=2024, leaf=1, streams=1, seed=0, m=1, sort_mode=None, flags=0,
         q=None, action=None, value=None, ws=None, h="env"):
    import torch

    p = lambda t: None if t is None else C.c_void_p(t if isinstance(t, int) else t.data_ptr())  # noqa: E731
    return env.L.mse_lookahead_net(env._h if h == "env" else h, None if policy is None else policy._h, horizon, gamma, base, det,
                                   base_seed, leaf, streams, seed, m, p(sort_mode), flags, p(q), p(action), p(value), p(ws),
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_nothing_else_is_touched():
    import torch

    GUARD, M_S = 64, 3
    env, twin, p = _env("mono", 0.05), _env("mono", 0.05), _policy("mono")
    A = env.num_actions
    sizes = {"q": 8 * A * N, "action": 4 * N, "value": 8 * N, "ws": int(env.L.mse_lookahead_workspace_bytes(env._h, M_S))}
    assert sizes["ws"] == 8 * M_S * A * N

    def buffers():
        at, off = {}, GUARD
        for name, size in sizes.items():
            at[name] = (off, size)
            off += (size + 15) // 16 * 16 + GUARD
        return torch.full((off,), 0xA5, dtype=torch.uint8, device="cuda"), at

    def inside(raw, at, names):
        m = torch.zeros(raw.numel(), dtype=torch.bool, device="cuda")
        for name in names:
            m[at[name][0]:at[name][0] + at[name][1]] = True
        return m

    before, t0, errors = _state_bits(env), env.policy_step, env.error_count()
    fwd = {k: v.clone() for k, v in p.forward(env.obs, env.mask, seed=4, t=2).items()}
    raw, at = buffers()
    ptr = {k: raw.data_ptr() + at[k][0] for k in at}
    kw = dict(horizon=4, gamma=0.9, base=2, det=0, base_seed=9, leaf=1, streams=1, seed=11, m=M_S)
    assert _raw(env, p, q=ptr["q"], action=ptr["action"], value=ptr["value"], ws=ptr["ws"], **kw) == 0
    torch.cuda.synchronize()
    assert bool((raw[~inside(raw, at, at)] == 0xA5).all()), "a guard byte was written"
    assert _same_state(before, env) and env.policy_step == t0 and env.error_count() == errors
    # action_out = value_out = NULL: q is the same, the two are not written
    raw2, at2 = buffers()
    ptr2 = {k: raw2.data_ptr() + at2[k][0] for k in at2}
    assert _raw(env, p, q=ptr2["q"], ws=ptr2["ws"], **kw) == 0
    torch.cuda.synchronize()
    assert bool((raw2[~inside(raw2, at2, ("q", "ws"))] == 0xA5).all())
    assert torch.equal(raw2[inside(raw2, at2, ("q",))], raw[inside(raw, at, ("q",))])
    # a rerun gives equal bits
    raw3, at3 = buffers()
    ptr3 = {k: raw3.data_ptr() + at3[k][0] for k in at3}
    assert _raw(env, p, q=ptr3["q"], action=ptr3["action"], value=ptr3["value"], ws=ptr3["ws"], **kw) == 0
    torch.cuda.synchronize()
    assert torch.equal(raw3, raw)
    # and the method returns the same bits as the raw call
    la = env.lookahead(4, gamma=0.9, base_policy=p, base_deterministic=False, leaf_value=p, base_seed=9, streams="fresh", seed=11,
                       n_samples=M_S)
    q_raw = raw[at["q"][0]:at["q"][0] + at["q"][1]].view(torch.int64)
    assert torch.equal(la["q"].view(torch.int64).reshape(-1), q_raw)
    # the policy handle is as it was: its forward gives the bits it gave
    again = p.forward(env.obs, env.mask, seed=4, t=2)
    assert all(torch.equal(fwd[k], again[k]) for k in fwd)
    # a following rollout() gives the bits it gives without the lookahead call
    got, exp = env.rollout(6, policy_seed=3), twin.rollout(6, policy_seed=3)
    torch.cuda.synchronize()
    for key in got:
        assert torch.equal(got[key].view(torch.uint8), exp[key].view(torch.uint8)), key
    assert all(torch.equal(a, b) for a, b in zip(env.get_state(), twin.get_state()))


def test_weights_are_read_at_launch():
    import marl_sortingenv_amd as M

    env, p = _env("mono", 0.05), _policy("mono", seed=3)
    kw = dict(horizon=3, gamma=0.9, streams="fresh", seed=1, base_seed=5, base_policy=p, leaf_value=p)
    first = {k: v.clone() for k, v in env.lookahead(**kw).items()}
    p.load_weights(_policy("mono", seed=11).flat_weights())
    second = _compare(env, "mono reloaded", **kw)  # equals the twin under the new weights
    assert not _same_bits(first, second)
    assert bool((first["q"] != second["q"]).any())
    assert isinstance(p, M.MlpPolicy)


def test_refusals_in_the_headers_order():
    import torch

    import marl_sortingenv_amd as M
    from marl_sortingenv_amd.config import SortingEnvConfig

    env = _env("mono", 0.0, n=64, warm=2)
    press = _env("press", 0.0, n=64, warm=2)
    p, wrong = _policy("mono"), _policy("press")
    general = SortingEnvConfig().with_overrides({"simulation": {"input_batch_size": 90}})
    # a handle that every handle-side refusal applies to: general generator mode, literal_choice, not reset
    worst = M.BatchedSortingEnv("mono", num_envs=64, max_steps=MAX_STEPS, noise_sorting=0.0, config=general, literal_choice=True,
                                reset_now=False)
    A = env.num_actions
    q = torch.full((A * 64 + 1,), 7.0, dtype=torch.float64, device="cuda")
    ws = torch.full((A * 64 + 1,), 7.0, dtype=torch.float64, device="cuda")
    val = torch.full((65,), 7.0, dtype=torch.float64, device="cuda")
    act = torch.full((64,), 7, dtype=torch.int32, device="cuda")
    sm = torch.zeros(64, dtype=torch.int32, device="cuda")
    ok = dict(q=q, action=act, value=val, ws=ws)
    L = env.L
    odd = lambda t: t.data_ptr() + 4  # noqa: E731  4 mod 8

    def refused(status, word, e=worst, policy=None, **kw):
        assert _raw(e, policy, **dict(ok, **kw)) == status, (word, L.mse_last_error())
        assert word.encode() in L.mse_last_error(), (word, L.mse_last_error())
        assert b"mse_lookahead_net" in L.mse_last_error()

    # each call is wrong in what it names AND in everything the header lists after it (arguments, policy and handle): the
    # earlier refusal wins
    later = dict(horizon=0, m=0, gamma=2.0, base=3, flags=1, sort_mode=sm, leaf=2, q=odd(q))
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
    refused(INVALID, "streams", **dict(later, base=2, streams=2))
    later.pop("base")
    for f in (1, 4, 8, 2 | 4):  # MSE_STEP_UNMASKED, MSE_ROLLOUT_RULE_BASED, MSE_STEP_SANITIZE_LATE
        refused(INVALID, "MSE_STEP_CHECK_OVERFLOW", **dict(later, flags=f))
    later.pop("flags")
    refused(INVALID, "sort_mode_dev", **later)
    later.pop("sort_mode")
    refused(INVALID, "policy is NULL", **later)
    refused(INVALID, "obs_dim -> num_actions", policy=wrong, **later)
    refused(INVALID, "leaf_value", policy=p, **later)
    refused(INVALID, "leaf_value", policy=p, **dict(later, leaf=-1))
    later.pop("leaf")
    for base in (0, 1):
        refused(INVALID, "mse_lookahead is the call", policy=p, base=base, leaf=0, **later)
    refused(UNSUPPORTED, "general generator mode", policy=p, **later)
    literal_cold = M.BatchedSortingEnv("mono", num_envs=64, max_steps=MAX_STEPS, noise_sorting=0.0, literal_choice=True, reset_now=False)
    refused(UNSUPPORTED, "literal_choice", e=literal_cold, policy=p, **later)
    cold = M.BatchedSortingEnv("mono", num_envs=64, max_steps=MAX_STEPS, noise_sorting=0.0, reset_now=False)
    refused(NOT_RESET, "mse_reset", e=cold, policy=p, **later)
    refused(ALIGNMENT, "8-byte", e=env, policy=p, **later)
    refused(ALIGNMENT, "8-byte", e=env, policy=p, value=odd(val))
    refused(ALIGNMENT, "8-byte", e=env, policy=p, ws=odd(ws))
    # on handles that are in order, the same refusals by name
    literal = M.BatchedSortingEnv("mono", num_envs=64, max_steps=MAX_STEPS, noise_sorting=0.0, literal_choice=True)
    refused(UNSUPPORTED, "literal_choice", e=literal, policy=p)
    gen = M.BatchedSortingEnv("mono", num_envs=64, max_steps=MAX_STEPS, noise_sorting=0.0, config=general)
    refused(UNSUPPORTED, "general generator mode", e=gen, policy=p)
    refused(INVALID, "obs_dim -> num_actions", e=press, policy=p)
    refused(INVALID, "policy is NULL", e=env)
    torch.cuda.synchronize()
    assert bool((q == 7.0).all()) and bool((ws == 7.0).all()) and bool((val == 7.0).all()) and bool((act == 7).all())
    # the accepted forms next to them
    assert _raw(press, wrong, sort_mode=sm, q=q, ws=ws, flags=2) == 0
    assert _raw(env, p, horizon=1, gamma=0.0, m=1, **ok) == 0 and _raw(env, p, gamma=1.0, base=2, leaf=0, streams=0, **ok) == 0
    assert _raw(env, p, base=0, leaf=1, det=7, **ok) == 0 and _raw(env, p, base=1, leaf=1, det=-1, **ok) == 0
    for e in (literal, gen):
        with pytest.raises(M.MseError):
            e.lookahead(2, leaf_value=p)


def test_collector_equals_its_docstrings_loop():
    """Expert iteration's collection: the student steps the env and is the base policy and the leaf value of the planner."""
    import torch

    import marl_sortingenv_amd as M
    from marl_sortingenv_amd.learner import _ptr, _stream

    K, H, GAMMA, SEED = 7, 3, 0.95, 40
    a, b = _env("mono", 0.05, max_steps=5, warm=0), _env("mono", 0.05, max_steps=5, warm=0)
    p = _policy("mono", seed=9)
    kw = dict(base_policy=p, leaf_value=p, base_deterministic=False, streams="fresh", base_seed=12, n_samples=2)
    col = M.LookaheadCollector(a, K, H, actor=p, gamma=GAMMA, seed=SEED, **kw)
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
        exp["stepped_actions"][k] = p.forward(b.obs, b.mask, seed=SEED, t=k, deterministic=False, index_offset=b.index_offset)["action"]
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
    assert bool(got["episode_starts"].any()) and bool((got["stepped_actions"] != got["actions"]).any())
    # the planner used the network: the rule base with no leaf labels differently
    plain = M.LookaheadCollector(_env("mono", 0.05, max_steps=5, warm=0), K, H, actor=p, gamma=GAMMA, seed=SEED, base_policy="rule_based",
                                 streams="fresh", base_seed=12, n_samples=2).collect()
    assert torch.equal(plain["stepped_actions"], got["stepped_actions"]) and not torch.equal(plain["values"], got["values"])
    # one ImitationLearner.update() of the student on its own planner's labels
    stats = M.ImitationLearner(p, batch_size=512, seed=1).update(got)["mean"]
    print("update:", stats)
    assert all(v == v and abs(v) != float("inf") for k, v in stats.items() if k != "_") and stats["unusable"] == 0


def test_evaluate_lookahead_equals_hand_loop():
    import torch

    import marl_sortingenv_amd as M
    from marl_sortingenv_amd.episodes import eval_targets

    n, max_steps, H, episodes = 10, 30, 2, 25
    p = _policy("mono")
    a = M.BatchedSortingEnv("mono", num_envs=n, base_seed=100, max_steps=max_steps, noise_sorting=0.0)
    b = M.BatchedSortingEnv("mono", num_envs=n, base_seed=100, max_steps=max_steps, noise_sorting=0.0)
    mean, std = M.evaluate_lookahead(a, episodes, H, streams="fresh", n_samples=2, seed=6, gamma=0.9, leaf_value=p)
    # the hand loop: SB3's counting rule through EpisodeStats
    b.reset(seeds=b.seeds)
    b.policy_step = 0
    targets = eval_targets(episodes, n)
    stats = M.EpisodeStats(n, b.device, slots=max(targets), targets=targets)
    buf = {"reward": torch.empty((max_steps, n), device="cuda"), "done": torch.empty((max_steps, n), dtype=torch.uint8, device="cuda")}
    t = 0
    for _ in range(max(targets)):
        for k in range(max_steps):
            la = b.lookahead(H, streams="fresh", n_samples=2, seed=6 + t, gamma=0.9, leaf_value=p)
            _, rew, done, _ = b.step(la["action"])
            buf["reward"][k], buf["done"][k] = rew, done
            t += 1
        stats.update(buf)
    s = stats.summary()
    print(f"evaluate_lookahead with the leaf: {mean} +- {std} over {s['episodes']} episodes")
    assert s["episodes"] == episodes
    assert mean == s["mean_return"] and std == s["std_return"]
    assert all(torch.equal(x, y) for x, y in zip(a.get_state(), b.get_state()))
