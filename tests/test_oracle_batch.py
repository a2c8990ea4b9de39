"""The batched oracle (orc_batch_*, oracle.OracleBatch) against N scalar OracleEnv objects, and the env-level seeding
at large seeds against the installed NumPy.

OracleBatch is what the full-size GPU tests (tests/test_gpu_full_size_oracle.py) hold every env to, so it must be the
scalar oracle exactly: every output of every step, the full snapshot, with one thread and with several."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import policy_stream as ps

A_OF = {"sort": 2, "press": 11, "mono": 22}


def _scalar_step(envs, actions, sort_mode, how):
    out = {k: [] for k in ("obs", "terminal_obs", "mask_pre", "mask", "reward", "term")}
    for i, o in enumerate(envs):
        out["mask_pre"].append(o.action_masks())
        eo, er, et = o.step(int(actions[i]), -1 if sort_mode is None else int(sort_mode[i]), **how)
        out["terminal_obs"].append(eo)
        if et:
            eo = o.reset(None)
        out["obs"].append(eo)
        out["mask"].append(o.action_masks())
        out["reward"].append(er)
        out["term"].append(int(et))
    return {k: np.asarray(v) for k, v in out.items()}


def _assert_snapshots_equal(batch, envs, tag):
    I, D, R = batch.snapshot()
    for i, o in enumerate(envs):
        ei, ed, er = o.snapshot()
        assert np.array_equal(I[i], ei), (tag, i, np.flatnonzero(I[i] != ei))
        assert np.array_equal(D[i].view(np.uint64), ed.view(np.uint64)), (tag, i)
        assert np.array_equal(R[i], er), (tag, i, np.flatnonzero(R[i] != er))


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("kind,noise,how", [
    ("mono", 0.0, dict()),
    ("mono", 0.05, dict()),
    ("mono", 0.05, dict(use_action_masking=False, sanitize_late=True)),
    ("mono", 0.0, dict(use_action_masking=False)),
    ("mono", 0.05, dict(check_overflow=True)),
    ("press", 0.05, dict()),
    ("press", 0.0, dict(use_action_masking=False, check_overflow=True)),
    ("sort", 0.05, dict()),
    ("sort", 0.0, dict(check_overflow=True)),
])
def test_batch_equals_scalar_envs(kind, noise, how, threads):
    """37 envs x 60 steps, max_steps 14: every env auto-resets four times (the unseeded rule); per-env sort_mode for
    Env_2 with -1 (the reference's rule) mixed in; a partial seeded and a partial unseeded reset halfway."""
    n, T, base, A = 37, 60, 9000, A_OF[kind]
    batch = O.OracleBatch(kind, n, base_seed=base, max_steps=14, noise_sorting=noise, threads=threads)
    envs = [O.OracleEnv(kind=kind, max_steps=14, seed=base + i, noise_sorting=noise) for i in range(n)]
    assert batch.obs_dim == envs[0].obs_dim and batch.num_actions == A
    assert np.array_equal(batch.obs(), np.stack([o.obs() for o in envs]))
    _assert_snapshots_equal(batch, envs, "create")
    rng = np.random.default_rng(5)
    masked = how.get("use_action_masking", True)
    for t in range(T):
        if t == 30:
            which = (np.arange(n) % 3 == 0).astype(np.uint8)
            seeds = np.arange(n, dtype=np.uint64) + np.uint64(2**32 - 10)
            got = batch.reset(seeds=seeds, which=which)
            exp = [o.reset(int(seeds[i])) if which[i] else o.obs() for i, o in enumerate(envs)]
            assert np.array_equal(got.view(np.uint32), np.stack(exp).view(np.uint32))
            which2 = (np.arange(n) % 4 == 1).astype(np.uint8)
            got = batch.reset(seeds=None, which=which2)
            exp = [o.reset(None) if which2[i] else o.obs() for i, o in enumerate(envs)]
            assert np.array_equal(got.view(np.uint32), np.stack(exp).view(np.uint32))
        mask = batch.action_masks()
        assert np.array_equal(mask, np.stack([o.action_masks() for o in envs]))
        if masked:
            act = ps.masked_uniform(rng.integers(0, 2**32, n, dtype=np.uint64), mask)
        else:
            act = rng.integers(0, A, n).astype(np.int32)
        sm = rng.integers(-1, 3 if kind == "press" else 2, n).astype(np.int32) if kind == "press" else None
        if kind == "press":
            assert np.array_equal(batch.sort_agent_obs().view(np.uint32),
                                  np.stack([o.sort_agent_obs() for o in envs]).view(np.uint32))
        got = batch.step(act, sort_mode=sm, want_terminal_obs=True, **how)
        exp = _scalar_step(envs, act, sm, how)
        for key in ("obs", "terminal_obs"):
            assert np.array_equal(got[key].view(np.uint32), exp[key].view(np.uint32)), (t, key)
        for key in ("mask_pre", "mask", "term"):
            assert np.array_equal(got[key], exp[key].astype(got[key].dtype)), (t, key)
        assert np.array_equal(got["reward"].view(np.uint64), exp["reward"].view(np.uint64)), t
        _assert_snapshots_equal(batch, envs, t)
    ints = batch.snapshot()[0]
    assert int(ints[:, O.SNAP["episode"]].max()) >= 4  # several auto-resets happened


def test_batch_from_a_seed_array_and_refused_actions():
    seeds = np.array([0, 2**32 - 1, 2**32, 2**63 - 1, 2**64 - 100, 7], dtype=np.uint64)
    batch = O.OracleBatch("press", len(seeds), seeds=seeds, max_steps=9, threads=3)
    envs = [O.OracleEnv(kind="press", max_steps=9, seed=int(s)) for s in seeds]
    _assert_snapshots_equal(batch, envs, "create")
    with pytest.raises(ValueError, match="env 2"):
        batch.step(np.array([0, 0, 11, 0, 0, 0]))


# ---- env-level seeding at large seeds, pinned to NumPy --------------------------------------------------------------

LARGE_SEEDS = list(range(2**32 - 100, 2**32 + 2)) + [2**40 + 7, 2**63 - 1]


def _state_words(gen):
    st = gen.bit_generator.state
    s, inc = int(st["state"]["state"]), int(st["state"]["inc"])
    m = (1 << 64) - 1
    return [s >> 64, s & m, inc >> 64, inc & m, int(st["has_uint32"]), int(st["uinteger"])]


@pytest.mark.parametrize("via", ["create", "reset"])
def test_env_streams_at_large_seeds_equal_numpy(via):
    """reset(seed) seeds rng_sorting, rng_pressing, rng_noise and rng from default_rng(seed + 2 / + 3 / + 4 / + 99)
    (env_super.py:165-184) and the input generator from default_rng(seed) followed by permutation([1, 2])
    (utils/input_generator.py:26-30): the snapshot's stream words equal NumPy's generator states, across 2**32 (where
    the seed's high word appears) and up to 2**63 - 1."""
    seeds = np.array(LARGE_SEEDS, dtype=np.uint64)
    if via == "create":
        batch = O.OracleBatch("mono", len(seeds), seeds=seeds, threads=2)
    else:
        batch = O.OracleBatch("mono", len(seeds), base_seed=3, threads=2)
        batch.step(np.zeros(len(seeds), dtype=np.int32))  # move every stream off its seeded state first
        batch.reset(seeds=seeds)
    ints, _, rng = batch.snapshot()
    for i, seed in enumerate(LARGE_SEEDS):
        for off, col in ((99, 0), (4, 6), (3, 12), (2, 18)):
            assert rng[i, col:col + 6].tolist() == _state_words(np.random.default_rng(seed + off)), (seed, off)
        g = np.random.default_rng(seed)
        first = int(g.permutation([1, 2])[0])
        assert rng[i, 24:30].tolist() == _state_words(g), seed
        assert int(ints[i, O.SNAP["gen_first"]][0]) == first, seed
        assert int(ints[i, O.SNAP["episode"]][0]) == 1


# ---- the host restatement of the policy stream ----------------------------------------------------------------------

@pytest.mark.parametrize("policy_seed", [0, 2024, 2**32 - 1, 2**32, 2**40 + 7, 2**64 - 1])
def test_policy_stream_drives_the_oracle_random_rollout_alike(policy_seed):
    """orc_env_random_rollout draws its masked-uniform actions from the C restatement of the stream (env index 0):
    stepping a twin with tests/policy_stream.py's draws gives the same trajectory, reward sum and final state."""
    kw = dict(kind="mono", max_steps=20, seed=11, noise_sorting=0.05)
    a, b = O.OracleEnv(**kw), O.OracleEnv(**kw)
    T = 90
    total = a.random_rollout(T, policy_seed=policy_seed)
    acc = 0.0
    key = ps.policy_key(policy_seed, np.zeros(1, dtype=np.uint64))
    for t in range(T):
        act = int(ps.masked_uniform(ps.policy_word(key, t), b.action_masks()[None, :])[0])
        obs, r, term = b.step(act)
        acc += r + float(obs[0])
        if term:
            b.reset(None)
    assert acc == total
    for x, y in zip(a.snapshot(), b.snapshot()):
        assert np.array_equal(x, y)


def test_masked_uniform_is_the_kth_valid_action():
    rng = np.random.default_rng(3)
    mask = rng.random((500, 22)) < 0.3
    mask[:, 0] = True
    mask[7] = False
    mask[7, 21] = True
    w = rng.integers(0, 2**32, 500, dtype=np.uint64)
    w[:3] = [0, 2**32 - 1, 2**31]
    got = ps.masked_uniform(w, mask)
    for i in range(500):
        valid = np.flatnonzero(mask[i])
        assert got[i] == valid[(int(w[i]) * len(valid)) >> 32]
    assert np.array_equal(ps.masked_uniform(w, mask, use_action_masking=False), ((w * np.uint64(22)) >> np.uint64(32)))
