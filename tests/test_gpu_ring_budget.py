"""PARITY (GPU): the ring kernels with no spare slots.

k_rollout_ring and k_rollout_policy_roles<RING = true> size their flow control by Params::ring_worst, admitted up to
kRingMaxPerStep = 31: two steps' draws take 62 of the ring's 64 slots.  The default config (ring_worst 19) never needs
more than about 36, so the other GPU tests would pass a ring that is only right with 26 slots to spare.  The configs of
tests/ring_budget.py put ring_worst at 0, 1, 2, 30, 31 (and 32: refused), and W1 / W30 / W31 / W31_batch120 draw exactly
ring_worst on consecutive steps (tests/test_ring_budget_cpu.py holds that on the oracle alone, for this batch).

Every step of every env is held to oracle.OracleBatch (tests/test_gpu_full_size_oracle.py's _run_rollouts: observations,
masks, done flags and actions on bits, the f32 reward by _check_reward, the state with the PCG64 position after every
launch), and buffers and state to a rollout_pipeline = 2 handle bit for bit.  300 envs: two workgroups, the second
ragged.  max_steps = 10 unless a case says otherwise; auto_reset on."""
import os

import numpy as np
import pytest

from tests import ring_budget as rb
from tests.test_gpu_full_size_oracle import _check_state, _np, _run_rollouts, _same, _start

pytestmark = pytest.mark.gpu

N = 300
# With max_steps = 10 the envs auto-reset inside steps 9, 19, 29, ... and the two steps after a reset draw nothing (the
# sorting stage is empty), so an RNG lane stands up to 2 x ring_worst = 62 outputs ahead when it hands the stream back
# there: the two-stage step back (d > 32).  Launch by launch (the step count after it):
LAUNCHES = (
    12,  # 12: ends 2 steps after a reset - the largest hand-back distance
    8,   # 20: ends 0 steps after a reset (the last step auto-resets)
    1,   # 21: K = 1, begins right after a reset, ends 1 step after it; nothing is drawn in the whole launch
    1,   # 22: K = 1, ends 2 steps after a reset, again nothing drawn
    2,   # 24: K = 2, both steps at the bound
    3,   # 27: K = 3
    13,  # 40: ends 0 steps after a reset
    16,  # 56: K = kRingTwoHalvesFrom: the observer lanes prime [worst, 2 worst); begins right after a reset
    15,  # 71: the longest launch primed in one half; ends 1 step after a reset
    17,  # 88: two halves, begins inside an episode
    2,   # 90: K = 2, ends 0 steps after a reset
    64,  # 154: begins right after a reset, six resets inside
)
POLICY_SEED = 2024
WIDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "marl-sortingenv_amd", "libmse_hip_widetie.so")


def _sort_mode(kind, n):
    """Env_2: arange(n) % 5 mapped to (-1, 0, 1, 2, 7) - the rule, both boosts, and two values that boost nothing"""
    import torch

    return torch.from_numpy(rb.press_sort_modes(n)) if kind == "press" else None


class _Twins:
    """A handle under test, its rollout_pipeline = 2 twin and the oracle, all on the same config, seeds and step count."""

    def __init__(self, name, kind, n=N, pipeline=3, max_steps=10, base_seed=0):
        self.b = rb.BUDGETS[name]
        self.tag = f"{name} {kind} n={n} pipeline={pipeline}"
        self.noise = self.b.noise
        self.env = self.b.env(kind, n, base_seed=base_seed, max_steps=max_steps, rollout_pipeline=pipeline)
        self.one = self.b.env(kind, n, base_seed=base_seed, max_steps=max_steps, rollout_pipeline=2)
        self.orc = self.b.oracle(kind, n, base_seed=base_seed, max_steps=max_steps)
        self.sm = _sort_mode(kind, n)
        self.launch = 0
        _start(self.tag, self.env, self.orc, self.noise)

    def rollouts(self, launches):
        import torch

        env, one = self.env, self.one
        buf = env.alloc_rollout(max(launches))
        env.alloc_rollout = lambda k_steps: buf  # _run_rollouts fills these, so that they can be compared below
        try:
            for K in launches:
                at = f"{self.tag} launch {self.launch} (K={K})"
                _run_rollouts(at, env, self.orc, self.noise, (K,), POLICY_SEED, sort_mode=self.sm)
                twin = one.rollout(K, policy_seed=POLICY_SEED, sort_mode=None if self.sm is None else self.sm.cuda())
                for key in twin:
                    assert torch.equal(buf[key][:K], twin[key][:K]), f"{at}: {key} differs from the one-lane kernel's"
                for x, y in zip(env.get_state(), one.get_state()):
                    assert torch.equal(x, y), f"{at}: state differs from the one-lane kernel's"
                self.launch += 1
        finally:
            del env.alloc_rollout
        assert env.policy_step == one.policy_step
        assert env.error_count() == 0 and one.error_count() == 0

    def partial_reset(self, which):
        """unseeded reset (streams continue) of the envs with which != 0, on all three"""
        import torch

        w = torch.from_numpy(which)
        obs, mask = self.env.reset(seeds=None, which=w)
        self.one.reset(seeds=None, which=w)
        exp = self.orc.reset(which=which)
        sel = np.flatnonzero(which)
        _same(f"{self.tag}: partial reset obs", _np(obs)[sel], exp[sel])
        _same(f"{self.tag}: partial reset mask", _np(mask)[sel], self.orc.action_masks()[sel])
        _check_state(f"{self.tag}: after the partial reset", self.env, self.orc, self.noise)


# ---- a. k_rollout_ring at the bound against the oracle --------------------------------------------------------------
RING_CASES = [(name, kind, N) for name in ("W31", "W30") for kind in ("mono", "press", "sort")] + \
             [(name, "mono", N) for name in ("W0", "W1", "W2", "W31_mixed", "W31_noise", "W31_batch120")] + \
             [("W31_press_noboost", "press", N), ("W31", "mono", 1)]


@pytest.mark.parametrize("name,kind,n", RING_CASES, ids=[f"{c[0]}-{c[1]}-{c[2]}" for c in RING_CASES])
def test_ring_rollout_at_the_bound_matches_the_oracle(name, kind, n):
    _Twins(name, kind, n).rollouts(LAUNCHES)


# ---- b. episodes that never draw ------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_steps", [1, 2, 3])
def test_ring_rollout_with_episodes_that_never_draw(max_steps):
    """max_steps 1 and 2: no step ever draws (an episode's first two steps find the sorting stage empty); 3: one step in
    three draws 31 or 9.  The RNG lanes still fill towards 2 x 31 outputs ahead and hand all of it back."""
    _Twins("W31", "mono", max_steps=max_steps).rollouts((1, 2, 3, 16, 5))


# ---- c. desynchronised lanes ----------------------------------------------------------------------------------------
def test_ring_rollout_with_desynchronised_lanes():
    """Two partial unseeded resets two steps apart: every wave then mixes lanes that draw 31 with lanes that draw 0 or 9,
    the wave-wide trip count M is set by the busiest lane and the idle lanes run ahead to their cap of r + 64 - the only
    place the hand-back distance reaches the ring's full depth."""
    t = _Twins("W31", "mono")
    t.rollouts((7,))
    t.partial_reset((np.arange(N) % 3 == 0).astype(np.uint8))
    t.rollouts((2,))
    t.partial_reset((np.arange(N) % 3 == 1).astype(np.uint8))
    t.rollouts((1, 2, 16, 3))


# ---- d. the learned-policy roles kernel with the ring ---------------------------------------------------------------
def _policy_case(name, kind, pipelines, collections=(16, 16, 3)):
    """FusedPolicyRollout, f16x3, on handles of the given rollout_pipeline values (0 picks k_rollout_policy_roles with
    the ring at this size when the config is eligible, 1 the roles without RNG waves, 2 the plain kernel): every buffer
    and the state bit-identical between them after each collection, and the first handle's state equal to an
    OracleBatch stepped with the collected actions."""
    import torch

    import marl_sortingenv_amd as M
    from tests.policy_head_reference import weights

    b = rb.BUDGETS[name]
    envs = [b.env(kind, N, base_seed=0, rollout_pipeline=p) for p in pipelines]
    orc = b.oracle(kind, N)
    tag = f"{name} {kind} policy"
    _start(tag, envs[0], orc, b.noise)
    w = weights(envs[0].obs_dim, envs[0].num_actions, seed=31)
    sm = _sort_mode(kind, N)
    K = max(collections)
    cols = [M.FusedPolicyRollout(e, M.MlpPolicy(e.obs_dim, e.num_actions, w, device=0, precision="f16x3"), K, seed=5,
                                 sort_mode=None if sm is None else sm.cuda()) for e in envs]
    assert all(c.policy.precision == "f16x3" for c in cols)
    for it, steps in enumerate(collections):
        outs = [c.collect(steps) for c in cols]
        for p, out, e in zip(pipelines[1:], outs[1:], envs[1:]):
            for key in outs[0]:
                assert torch.equal(outs[0][key], out[key]), f"{tag} collection {it}: {key}, pipelines {pipelines[0]} / {p}"
            for x, y in zip(envs[0].get_state(), e.get_state()):
                assert torch.equal(x, y), f"{tag} collection {it}: state, pipelines {pipelines[0]} / {p}"
        acts = _np(outs[0]["actions"][:steps])
        for k in range(steps):
            _same(f"{tag} collection {it} step {k}: observation", _np(outs[0]["observations"][k]), orc.obs())
            _same(f"{tag} collection {it} step {k}: action mask", _np(outs[0]["action_masks"][k]), orc.action_masks())
            orc.step(acts[k], sort_mode=None if sm is None else sm.numpy())
        _check_state(f"{tag} collection {it}", envs[0], orc, b.noise)
    assert all(e.policy_step == sum(collections) for e in envs)
    assert all(e.error_count() == 0 for e in envs)


@pytest.mark.parametrize("kind", ["mono", "press"])
@pytest.mark.parametrize("name", ["W31", "W0", "W31_mixed"])
def test_policy_roles_kernel_with_the_ring_at_the_bound(name, kind):
    """(W31_mixed as Env_2 compiles to ring_worst 38 - its no-boost mode - so that one case runs the roles without the
    ring on all but the plain handle; tests/test_ring_budget_cpu.py pins which plan each config gets.)"""
    _policy_case(name, kind, (0, 2, 1))


# ---- e. over budget -------------------------------------------------------------------------------------------------
def test_ring_refuses_a_config_over_budget():
    from marl_sortingenv_amd._lib import MseError

    with pytest.raises(MseError, match="at most 31 draws per step"):
        rb.BUDGETS["W32"].env("mono", N, rollout_pipeline=3)


def test_over_budget_config_runs_on_the_two_role_kernel():
    """W32 by size (rollout_pipeline 0): k_rollout_po, against the oracle and the one-lane kernel"""
    _Twins("W32", "mono", pipeline=0).rollouts((12, 8, 1, 16, 3))


def test_over_budget_config_policy_rollout_equals_the_plain_kernel():
    _policy_case("W32", "mono", (0, 2))


# ---- f. wide tie window ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["W31", "W31_mixed"])
def test_wide_window_ring_at_the_bound_equals_shipped_literal(name):
    """The wide-window build (tests/test_gpu_widetie.py) sends ~3 % of the draws to the literal cdf, which the ring
    kernel serves by redoing the whole step on jump-ahead outputs - here with the step's consumption at the bound."""
    import torch

    import marl_sortingenv_amd as M

    assert os.path.exists(WIDE), "build libmse_hip_widetie.so first: python __graft_entry__.py"
    assert M.load_library(WIDE).mse_tie_window() == 0x08000000
    b = rb.BUDGETS[name]
    a = b.env("mono", N, base_seed=31, rollout_pipeline=3, library=WIDE)
    lit = b.env("mono", N, base_seed=31, rollout_pipeline=2, literal_choice=True)
    ra, rl = a.rollout(48, policy_seed=5), lit.rollout(48, policy_seed=5)
    for key in ra:
        assert torch.equal(ra[key], rl[key]), key
    for x, y in zip(a.get_state(), lit.get_state()):
        assert torch.equal(x, y)
    assert a.error_count() == 0
