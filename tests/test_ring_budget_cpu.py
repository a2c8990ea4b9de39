"""The ring kernels' draw budget pinned on the CPU (tests/ring_budget.py): what Params::ring_worst is for each named
config, that it bounds what a step of the oracle really draws, and that the configs built to attain it do - the
condition under which tests/test_gpu_ring_budget.py runs the ring with no spare slots.  Nothing here calls the engine:
consumption is counted by walking the main stream's LCG between oracle snapshots."""
import numpy as np
import pytest

import marl_sortingenv_amd as M
from tests import config_tables_reference as R
from tests import replay
from tests import ring_budget as rb
from tests.fuzz_configs import fuzz_overrides, meta_for
from tests.test_config_tables_cpu import _steps, check
from tests.test_config_tables_cpu import lib as tables_lib  # noqa: F401  (fixture: mse_tables.h compiled on the host)
from tests.test_rollout_plan import LIMIT, MSG_RING, OK, RING, ROLES, ROLES_RING, TWO_ROLE, UNSUPPORTED, plan_policy, plan_rollout
from tests.test_rollout_plan import lib as plan_lib  # noqa: F401  (fixture: mse_plan.h compiled on the host)

KINDS = ("mono", "press", "sort")
CUS = 256
POLICY_LDS = (LIMIT - 1024, LIMIT - 65536, 21264, 4096, 6144, 10240)  # every kernel's image fits
GPU_N, GPU_MAX_STEPS, GPU_BASE_SEED = 300, 10, 0  # the batch tests/test_gpu_ring_budget.py launches


# ---- ring_worst of the named configs -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(rb.BUDGETS))
def test_named_config_compiles_to_its_ring_worst(tables_lib, plan_lib, name, kind):
    b = rb.BUDGETS[name]
    want = rb.reference_worst(b.sorting_config(), b.noise, kind)
    assert want == b.expected_worst(kind)  # (Env_2's no-boost mode costs W31_mixed and W31_noise more: 38, 32)
    P, _, literal, noise_on = check(tables_lib, b.struct(kind))
    assert P.ring_worst == want and (P.gen_mode, literal, noise_on) == (0, False, b.noise != 0.0)
    # ring_fwd is ring_worst single steps of the LCG; for W0 the identity map
    s, inc = 0x0123456789ABCDEF0F1E2D3C4B5A6978, 0xFEDCBA9876543210A5A5A5A5DEADBEEF | 1
    fwd = (P.ring_fwd[0] | (P.ring_fwd[1] << 64), P.ring_fwd[2] | (P.ring_fwd[3] << 64))
    assert R.lcg_apply(fwd, s, inc) == _steps(s, inc, want)
    if want == 0:
        assert fwd == (1, 0) and list(P.ring_fwd) == [1, 0, 0, 0]
    # the kernel the plan selects with that number
    args = (GPU_N, CUS, 0, 0, P.ring_worst, LIMIT - 1024, 1)
    pol = plan_policy(plan_lib, 0, GPU_N, CUS, 1, 0, P.ring_worst, 0, 0, 1, POLICY_LDS)
    if want <= rb.RING_MAX_PER_STEP:
        assert plan_rollout(plan_lib, 3, *args) == (RING, OK, None) and plan_rollout(plan_lib, 0, *args) == (RING, OK, None)
        assert pol[:2] == (ROLES_RING, OK)
    else:
        assert plan_rollout(plan_lib, 3, *args) == (None, UNSUPPORTED, MSG_RING)
        assert plan_rollout(plan_lib, 0, *args) == (TWO_ROLE, OK, None)
        assert pol[:2] == (ROLES, OK)


def test_the_named_configs_sit_where_they_should():
    assert {n: b.worst for n, b in rb.BUDGETS.items()} == dict(
        W0=0, W1=1, W2=2, W30=30, W31=31, W31_mixed=31, W31_press_noboost=31, W32=32, W31_noise=31, W31_batch120=31)
    assert rb.BUDGETS["W31_noise"].noise == 0.05 and all(b.noise == 0.0 for n, b in rb.BUDGETS.items() if n != "W31_noise")
    assert rb.pattern_counts(rb.BUDGETS["W31_batch120"].sorting_config())[1:] == [[48, 18, 42, 12], [18, 48, 12, 42]]
    assert "W32" not in rb.RING_ELIGIBLE and len(rb.RING_ELIGIBLE) == len(rb.BUDGETS) - 1


# ---- draws_per_step itself ---------------------------------------------------------------------------------------------
def test_draws_per_step_counts_lcg_steps():
    """on made-up snapshots: d steps of s' = M s + inc are found for d = 0..64, 65 and a changed increment are refused"""
    s, inc = 0x0123456789ABCDEF0F1E2D3C4B5A6978, 0xFEDCBA9876543210A5A5A5A5DEADBEEF | 1

    def snap(state):
        w = np.zeros(30, dtype=np.uint64)
        w[0:4] = [state >> 64, state & (2**64 - 1), inc >> 64, inc & (2**64 - 1)]
        return None, None, w

    for d in (0, 1, 2, 31, 32, 63, 64):
        assert rb.draws_per_step(None, snap(s), snap(_steps(s, inc, d))) == d
    with pytest.raises(AssertionError):
        rb.draws_per_step(None, snap(s), snap(_steps(s, inc, 65)))
    other = snap(s)
    other[2][3] += np.uint64(2)
    with pytest.raises(AssertionError):
        rb.draws_per_step(None, snap(s), other)


# ---- the bound is a bound ----------------------------------------------------------------------------------------------
def _consumption(orc, steps, sort_mode=None, seed=0):
    """[steps, N] outputs of the main stream consumed per step under random masked actions (auto-resets included)"""
    rng = np.random.default_rng(seed)
    n, A = orc.num_envs, orc.num_actions
    out = np.zeros((steps, n), dtype=np.int64)
    pre = orc.snapshot()
    for t in range(steps):
        mask = orc.action_masks()
        act = np.argmax(rng.random((n, A)) * mask, axis=1).astype(np.int32)  # uniform over the allowed actions
        assert mask[np.arange(n), act].all()
        orc.step(act, sort_mode=sort_mode)
        post = orc.snapshot()
        out[t] = rb.draws_per_step(orc, pre, post)
        pre = post
    return out


def _bound_cases():
    cases = [(f"{name}-{kind}", kind, name) for name in rb.BUDGETS for kind in KINDS]
    return cases + [(f"default-noise{noise}-{kind}", kind, noise) for noise in (0.0, 0.05) for kind in KINDS]


def _assert_bounded(tag, kind, worst, ocfg, max_steps):
    """3 episodes of 10 envs under random masked actions; Env_2's sort_mode cycles -1, 0, 1, 2, 7 over the envs"""
    from oracle.oracle import OracleBatch

    n = 10
    orc = OracleBatch(kind, n, base_seed=40, cfg=ocfg)
    d = _consumption(orc, 3 * max_steps, rb.press_sort_modes(n) if kind == "press" else None)
    assert d.max() <= worst, (tag, int(d.max()), worst)
    return d


@pytest.mark.parametrize("tag,kind,what", _bound_cases(), ids=[c[0] for c in _bound_cases()])
def test_no_step_draws_more_than_ring_worst(tag, kind, what):
    """Every named config (W32 and the over-budget press variants included: the bound is max_draws_per_step's, not the
    ring's) and the default config without and with noise."""
    from oracle.oracle import default_config

    if isinstance(what, str):
        b = rb.BUDGETS[what]
        worst, ocfg = rb.reference_worst(b.sorting_config(), b.noise, kind), b.oracle_config(kind, 25)
    else:
        worst, ocfg = rb.reference_worst(M.SortingEnvConfig(), what, kind), default_config(kind, 25, what, 200)
        assert worst == {("mono", 0.0): 19, ("sort", 0.0): 19, ("press", 0.0): 25, ("mono", 0.05): 23, ("sort", 0.05): 23,
                         ("press", 0.05): 31}[(kind, what)]
    _assert_bounded(tag, kind, worst, ocfg, 25)


def _ring_eligible_fuzz(kind):
    """[(seed, ring_worst, max_steps)] of the fuzz configs 0..45 the ring kernels serve: counts without a remainder, the
    integer draw path, at most 31 draws per step"""
    out = []
    for seed in range(46):
        ov, ctor = fuzz_overrides(seed)
        rc, _, P, _, literal, _ = R.compile_config(M.SortingEnvConfig().with_overrides(ov).to_struct(kind, **ctor), 1000, 0)
        if rc == R.OK and not (P["gen_mode"] or literal or P["ring_worst"] > rb.RING_MAX_PER_STEP):
            out.append((seed, P["ring_worst"], ctor["max_steps"]))
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_no_step_draws_more_than_ring_worst_under_the_fuzzed_configs(kind):
    eligible = _ring_eligible_fuzz(kind)
    assert eligible
    for seed, worst, max_steps in eligible:
        _assert_bounded(f"fuzz{seed}-{kind}", kind, worst, replay.oracle_config(meta_for(kind, seed)), max_steps)


def test_ring_eligible_fuzz_configs_exist():
    """several of seeds 0..45 are ring-eligible, seed 24 (mono, ring_worst 18: the one the GPU fuzz test reaches) among them"""
    mono = _ring_eligible_fuzz("mono")
    assert (24, 18) in [(s, w) for s, w, _ in mono] and len(mono) >= 3, mono


# ---- the bound is attained ---------------------------------------------------------------------------------------------
# The batch the GPU cases launch (300 envs from seed 0, max_steps 10), 70 steps of it.  An episode's first two steps draw
# nothing (the sorting stage is still empty), and each episode draws its season by a coin: in one season D has 35 (42)
# units and a step draws exactly ring_worst, in the other 10 (12) units and 9 (W1: 0).  So of the 8 drawing steps in 10,
# about half the envs are at the bound: ~40 % of all env-steps, on every batch step but the episodes' first two.
ATTAIN_STEPS = 70


@pytest.fixture(scope="module")
def attained():
    """name -> [ATTAIN_STEPS, GPU_N] consumption of every named config as Env_3 (W31_press_noboost as Env_2 under the
    GPU case's sort_mode vector)"""
    out = {name: _consumption(b.oracle("mono", GPU_N, GPU_BASE_SEED, GPU_MAX_STEPS), ATTAIN_STEPS)
           for name, b in rb.BUDGETS.items() if name != "W31_press_noboost"}
    out["W31_press_noboost"] = _consumption(rb.BUDGETS["W31_press_noboost"].oracle("press", GPU_N, GPU_BASE_SEED, GPU_MAX_STEPS),
                                            ATTAIN_STEPS, rb.press_sort_modes(GPU_N))
    return out


def test_what_the_named_configs_consume(attained):
    """the table of DESIGN.md 4.6, re-measured (run with -s to see it)"""
    for name, d in attained.items():
        values, counts = np.unique(d, return_counts=True)
        print(f"{name}: ring_worst {rb.BUDGETS[name].worst}, outputs per step -> env-steps: "
              f"{dict(zip(values.tolist(), counts.tolist()))}")
        assert d.max() <= rb.BUDGETS[name].worst
    assert attained["W0"].max() == 0
    assert set(np.unique(attained["W2"])) == {0, 2}
    assert attained["W32"].max() == 32  # attained: the config the ring must be refused


@pytest.mark.parametrize("name", rb.ATTAINED)
def test_the_bound_is_attained(attained, name):
    """On at least half of the batch's steps envs draw exactly ring_worst - in every wave of 64 envs - and envs do so on
    two consecutive steps (the case the ring's two-step margin is sized for).  Counted per env-step the share cannot
    reach a half on a whole batch: a coin per episode picks the season and two steps in ten draw nothing, so 0.5 x 0.8 =
    40 % is its expectation (measured: 39.7 % of 21 000, 7 301 consecutive pairs, 56 of 70 steps); a single env can lie
    above a half by luck.  The per-env-step share is held to a third: 40 % less seven standard deviations of a mean
    over 2 100 episodes (0.8 x sqrt(0.25 / 2100) = 0.9 %)."""
    d, worst = attained[name], rb.BUDGETS[name].worst
    hit = d == worst
    assert d.max() == worst
    waves = [slice(w, min(w + 64, GPU_N)) for w in range(0, GPU_N, 64)]
    steps_at_bound = np.array([[hit[t, w].any() for w in waves] for t in range(ATTAIN_STEPS)]).all(axis=1)
    assert steps_at_bound.sum() >= ATTAIN_STEPS / 2, int(steps_at_bound.sum())
    assert hit.mean() >= 1 / 3, float(hit.mean())
    pairs = hit[1:] & hit[:-1]
    assert pairs.any(axis=0).sum() >= GPU_N / 2, int(pairs.any(axis=0).sum())  # most envs, several times each
    # the season that is not at the bound, and the steps that draw nothing
    cfg = rb.BUDGETS[name].sorting_config()
    light = min(c[3] for c in rb.pattern_counts(cfg)[1:])
    other = light - int(np.rint(light * cfg.baseline_accuracy[3]))  # 9, 8 (W30) or 0 (W1)
    assert set(np.unique(d)) == {0, other, worst}
    print(f"{name}: ring_worst {worst}; exactly that on {hit.mean():.1%} of {d.size} env-steps, in every wave on "
          f"{int(steps_at_bound.sum())} of {ATTAIN_STEPS} steps; {int(pairs.sum())} consecutive pairs; else {other} or 0")
    assert (d[[0, 1]] == 0).all()


def test_the_press_noboost_config_draws_at_least_26_twice_running(attained):
    d = attained["W31_press_noboost"]
    assert d.max() <= 31
    heavy = d >= 26
    assert (heavy[1:] & heavy[:-1]).any(axis=0).sum() >= GPU_N / 2
