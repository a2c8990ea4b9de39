"""GPU: the all-env trace (mse_trace_begin_all).  Every env's record columns against that env's scalar oracle
(`OracleEnv.trace_record()`: integers exactly, the three reward columns within 1e-6, the project's reward bound) and against
a one-env `mse_trace_begin` run of a twin env (bit for bit), at N = 1, 65 (one lane past a wave) and 257 (one past the
256-lane pad), all three kinds, noise 0 and 0.05, stepped without masking and with check_overflow over auto-resets.  Then
the edges: guard cells behind capacity x 40 x N, the capacity refusal, mse_rollout refused, stepping after mse_trace_end
against an untraced twin, and the plant scan's carry against the engine's own O(1) bale ledger (mse_get_state)."""
import ctypes as C

import numpy as np
import pytest

from oracle.oracle import SNAP, OracleEnv
from tests import plant_reference as R

pytestmark = pytest.mark.gpu

STEPS, MAX_STEPS, BASE_SEED = 36, 13, 40
REWARD_COLS = [1, 2, 32]       # R_SORT, R_PRESS, REWARD
EXACT_COLS = [c for c in range(40) if c not in REWARD_COLS]  # integers, and the accuracy doubles the project holds bit for bit


def _env(kind, n, noise, **kw):
    import marl_sortingenv_amd as M

    return M.BatchedSortingEnv(kind=kind, num_envs=n, device=0, base_seed=BASE_SEED, max_steps=MAX_STEPS, noise_sorting=noise,
                               balesize=200, **kw)


def _actions(kind, n, noise):
    import marl_sortingenv_amd as M

    rng = np.random.default_rng(1000 * n + len(kind) + int(noise * 100))
    return rng.integers(0, M.NUM_ACTIONS[kind], (STEPS, n)).astype(np.int32)


@pytest.mark.parametrize("noise", [0.0, 0.05])
@pytest.mark.parametrize("kind", ["mono", "press", "sort"])
@pytest.mark.parametrize("n", [1, 65, 257])
def test_all_env_trace_against_oracle_and_one_env_trace(n, kind, noise):
    import torch

    acts = _actions(kind, n, noise)
    dev_acts = torch.from_numpy(acts).cuda()
    env = _env(kind, n, noise)
    env.trace_begin_all(STEPS)
    dones = []
    for k in range(STEPS):
        _, _, done, _ = env.step(dev_acts[k], use_action_masking=False, check_overflow=True)
        dones.append(done.cpu().numpy().copy())
    rec = env.trace_end().cpu().numpy()
    assert rec.shape == (STEPS, 40, n)
    dones = np.asarray(dones)
    assert np.array_equal(rec[:, R.DONE] != 0, dones != 0) and dones.sum() >= 2 * n, "the run must cross auto-resets"

    # every env against its scalar oracle
    for i in range(n):
        orc = OracleEnv(kind=kind, max_steps=MAX_STEPS, seed=BASE_SEED + i, noise_sorting=noise, balesize=200)
        orc.reset(BASE_SEED + i)
        for k in range(STEPS):
            _, _, term = orc.step(int(acts[k, i]), use_action_masking=False, check_overflow=True)
            want, got = orc.trace_record(), rec[k, :, i]
            assert np.array_equal(got[EXACT_COLS], want[EXACT_COLS]), (i, k, got, want)
            assert np.all(np.abs(got[REWARD_COLS] - want[REWARD_COLS]) <= 1e-6), (i, k, got[REWARD_COLS], want[REWARD_COLS])
            if term:
                orc.reset()
        orc.close()

    # the one-env trace of a twin env, bit for bit
    for i in sorted({0, 63, 64, n - 1} & set(range(n))):
        twin = _env(kind, n, noise)
        twin.trace_begin(i, STEPS)
        for k in range(STEPS):
            twin.step(dev_acts[k], use_action_masking=False, check_overflow=True)
        one = twin.trace_end().cpu().numpy()
        assert one.shape == (STEPS, 40) and np.array_equal(one.view(np.uint64), np.ascontiguousarray(rec[:, :, i]).view(np.uint64)), i
        twin.close()
    env.close()


@pytest.mark.parametrize("n", [65, 257])
def test_guards_capacity_rollout_refusal_and_life_after_the_trace(n):
    import torch

    import marl_sortingenv_amd as M

    kind, noise, cap = "mono", 0.05, 9
    acts = torch.from_numpy(_actions(kind, n, noise)).cuda()
    env, twin = _env(kind, n, noise), _env(kind, n, noise)
    L, p = env.L, lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    cells, band = cap * 40 * n, 4096
    buf = torch.full((cells + band,), -777.0, dtype=torch.float64, device="cuda")
    assert L.mse_trace_begin_all(env._h, p(buf), cap) == 0
    for k in range(cap):
        env.step(acts[k], use_action_masking=False, check_overflow=True)
        twin.step(acts[k], use_action_masking=False, check_overflow=True)
    torch.cuda.synchronize()
    assert bool((buf[cells:] == -777.0).all()), "cells behind capacity x 40 x N were written"
    planes = buf[:cells].view(cap, 40, n)
    assert bool((planes[:, :38] != -777.0).all()) and bool((planes[:, 38:] == -777.0).all())  # columns 38, 39 are not written
    # a step past the capacity is refused, and refused before anything runs
    state = [t.clone() for t in env.get_state()]
    with pytest.raises(M.MseError, match="trace buffer is full"):
        env.step(acts[cap], use_action_masking=False, check_overflow=True)
    assert all(torch.equal(a, b) for a, b in zip(state, env.get_state()))
    # mse_rollout is refused while the trace is attached
    with pytest.raises(M.MseError, match="a trace is attached"):
        env.rollout(4)
    count = C.c_int64(-1)
    assert L.mse_trace_end(env._h, C.byref(count)) == 0 and count.value == cap
    assert L.mse_trace_end(env._h, C.byref(count)) == 0 and count.value == 0
    # after the trace the env steps like a twin that never had one
    for k in range(cap, cap + 6):
        a = env.step(acts[k], use_action_masking=False, check_overflow=True, want_reward64=True)
        b = twin.step(acts[k], use_action_masking=False, check_overflow=True, want_reward64=True)
        assert all(torch.equal(x, y) for x, y in zip(a, b)) and torch.equal(env.reward64, twin.reward64)
    assert all(torch.equal(a, b) for a, b in zip(env.get_state(), twin.get_state()))
    assert bool((buf[cells:] == -777.0).all())
    env.rollout(4)  # and rollouts are served again
    # begin_all's own refusals
    assert L.mse_trace_begin_all(env._h, None, cap) == -1 and L.mse_trace_begin_all(env._h, p(buf), 0) == -1
    assert L.mse_trace_begin_all(None, p(buf), cap) == -1
    env.close()
    twin.close()


def test_plant_carry_equals_the_engines_bale_ledger():
    """Mid-episode, the scan's carry (bales, mass, last size per material) equals the bale_* columns of mse_get_state:
    two O(1) forms of the same lists, one kept by the step kernel, one rebuilt from the trace."""
    import torch

    import marl_sortingenv_amd as M
    from marl_sortingenv_amd.plant import PlantStats, plant_params

    n = 257
    env = M.BatchedSortingEnv(kind="mono", num_envs=n, device=0, base_seed=3, max_steps=60, noise_sorting=0.05, balesize=150)
    assert plant_params(env) == (150, 75)
    stats = PlantStats(env, n)
    seen_bales = 0
    for chunk in range(3):
        env.trace_begin_all(17)
        for k in range(17):
            env.step(env.sample_actions(7))
        stats.update(env.trace_end())
        torch.cuda.synchronize()
        ints = env.get_state()[0].cpu().numpy()
        run = stats.run.cpu().numpy()
        assert np.array_equal(run[0], ints[:, SNAP["current_step"]].reshape(-1)), "the carry's length is the env's current_step"
        assert np.array_equal(run[10:15].T, ints[:, SNAP["bale_count"]])
        assert np.array_equal(run[15:20].T, ints[:, SNAP["bale_sum"]])
        assert np.array_equal(run[30:35].T, ints[:, SNAP["bale_last_size"]])
        seen_bales = int(run[10:15].sum())
    print("bales in the carry at the end:", seen_bales)
    assert seen_bales > 0, "the envs must have pressed bales"
    env.close()
