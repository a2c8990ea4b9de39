"""GPU: the labelled policy rollout (mse_rollout_policy_labelled, FusedPolicyRollout(expert_labels=True)) - PPO's own
on-policy rollout with the rule-based controller's label of every recorded state, K steps per launch - against

  * FusedPolicyRollout on an identically constructed env: the nine outputs, the full state and the policy step counter;
  * PolicyRolloutCollector(expert_labels=True), the multi-launch twin, and the sentence of include/mse.h written out here
    (`hand_labels`: rule_actions() before each step of the recorded actions) for `expert_actions`;
  * guard bytes, NULL outputs, every refusal with its check-only form, and the learner's loop.

All comparisons are on bits.  max_steps = 3 puts episode ends inside and across the launches.
Label quality (asserted, not assumed): on the mono cases with max_steps = 40 the rollout is continued to the episode's 40
steps and the share of labels the recorded mask forbids must lie above 0 and below 0.25 wherever there are at least 33 envs
(1 320 labels; one env's 40 labels are printed only: DESIGN 4.16 / 4.17 measured 0.04 - 0.10, two to four labels)."""
import ctypes as C

import numpy as np
import pytest

from tests.rollout_checks import bits_equal, cus, guarded, inside, overflow_config
from tests.test_gpu_demo_rollout import BIG_TABLES, DIMS, GEN, _actor, _env
from tests.test_gpu_model_rollout import _state_equal

pytestmark = pytest.mark.gpu

SEED = 77
NINE = ("observations", "action_masks", "actions", "log_probs", "values", "rewards", "episode_starts", "last_values", "last_dones")
LAUNCHES = (5, 1, 4)


def hand_labels(env, actions):
    """rule_actions() of the state before each step of `actions` (i32[K, N]) on `env` -> i32[K, N]"""
    import torch

    out = torch.empty_like(actions)
    for k in range(actions.shape[0]):
        out[k].copy_(env.rule_actions())
        env.step(actions[k])
    return out


def illegal_share(labels, masks):
    return float((masks.gather(2, labels.long().unsqueeze(2)).squeeze(2) == 0).float().mean())


def _compare(tag, kind, n, noise, max_steps, precision, det, launches=LAUNCHES, flags=None, **kw):
    """-> (labels, masks) of all launches.  Four identically constructed envs: labelled, plain fused, the twin, the hand loop."""
    import torch

    import marl_sortingenv_amd as M

    pol = _actor(kind, precision)
    a, b, c, d = (_env(kind, n, noise, max_steps, **kw) for _ in range(4))
    collect_kw = flags or {}
    labels, masks, last_dones = [], [], None
    for K in launches:
        t0 = a.policy_step
        got = M.FusedPolicyRollout(a, pol, K, seed=SEED, expert_labels=True).collect(deterministic=det, **collect_kw)
        exp = M.FusedPolicyRollout(b, pol, K, seed=SEED).collect(deterministic=det, **collect_kw)
        assert "expert_actions" not in exp and got["expert_actions"].dtype == torch.int32 and got["expert_actions"].shape == (K, n)
        bits_equal(f"{tag} K={K}", got, exp, keys=NINE)
        _state_equal(f"{tag} K={K}", a, b)
        assert a.policy_step == t0 + K
        if not collect_kw:  # the twin offers neither flag; the hand loop serves those
            twin = M.PolicyRolloutCollector(c, pol, K, seed=SEED, expert_labels=True)
            if last_dones is not None:  # a stepped handle: the twin carries t and the last dones itself
                twin.t = t0
                twin._last_done.copy_(last_dones)
            tw = twin.collect(deterministic=det)
            bits_equal(f"{tag} K={K} twin", got, tw, keys=NINE[:7] + ("expert_actions", "last_values", "last_dones"))
            last_dones = tw["last_dones"]
            assert torch.equal(got["expert_actions"], hand_labels(d, got["actions"])), f"{tag} K={K}: labels against the hand loop"
        labels.append(got["expert_actions"].clone())
        masks.append(got["action_masks"].clone())
    assert a.error_count() == 0 or collect_kw
    for e in (a, b, c, d):
        e.close()
    return torch.cat(labels), torch.cat(masks)


# ---- 1. every kind, size, noise, episode length, precision form and sampling mode -------------------------------------------
@pytest.mark.parametrize("det", [False, True], ids=["sampled", "argmax"])
@pytest.mark.parametrize("precision", ["f16x3", "f32"])
@pytest.mark.parametrize("max_steps", [3, 40])
@pytest.mark.parametrize("noise", [0.0, 0.05], ids=["n0", "n5"])
@pytest.mark.parametrize("n", [1, 33, 257])
@pytest.mark.parametrize("kind", ["sort", "press", "mono"])
def test_labelled_rollout_matches_the_plain_rollout_the_twin_and_the_hand_loop(kind, n, noise, max_steps, precision, det):
    launches = LAUNCHES + ((30,) if kind == "mono" and max_steps == 40 else ())  # ... to the episode's end: label quality
    labels, masks = _compare(f"{kind} n={n} noise={noise} T={max_steps} {precision} det={det}", kind, n, noise, max_steps,
                             precision, det, launches=launches)
    if kind == "mono" and max_steps == 40:
        share = illegal_share(labels, masks)
        print(f"mono n={n} noise={noise} {precision} det={det}: {share:.4f} of {labels.numel()} labels are illegal under the recorded mask")
        if n >= 33:
            assert 0.0 < share < 0.25, share


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_labelled_rollout_in_64_env_waves(precision):
    _compare(f"tiles=2 {precision}", "mono", 256 * cus() + 1, 0.05, 3, precision, False, launches=(2,))


def test_labelled_rollout_on_a_shard():
    """index_offset enters the policy's stream keys, not the label"""
    _compare("index_offset", "mono", 33, 0.05, 3, "f16x3", False, index_offset=2 ** 32 + 5)


@pytest.mark.parametrize("kind", ["press", "mono"])
def test_labelled_rollout_flags(kind):
    """MSE_STEP_UNMASKED and MSE_STEP_CHECK_OVERFLOW: the outputs and the state are the plain rollout's under the same flag,
    and the labels are rule_actions() of the states that rollout passes through"""
    import torch

    import marl_sortingenv_amd as M

    pol = _actor(kind)
    for collect_kw, env_kw in ((dict(use_action_masking=False), {}), (dict(check_overflow=True), dict(config=overflow_config(0.05)))):
        _compare(f"{kind} {collect_kw}", kind, 97, 0.05, 3, "f16x3", False, flags=collect_kw, **env_kw)
        # the labels under the flag: a hand loop that steps the recorded actions with the same flag
        a, d = _env(kind, 97, **env_kw), _env(kind, 97, **env_kw)
        got = M.FusedPolicyRollout(a, pol, 10, seed=SEED, expert_labels=True).collect(**collect_kw)
        want = torch.empty_like(got["expert_actions"])
        for k in range(10):
            want[k].copy_(d.rule_actions())
            d.step(got["actions"][k], **collect_kw)
        assert torch.equal(got["expert_actions"], want)
        if "check_overflow" in collect_kw:  # tests/test_gpu_demo_rollout.py's criterion: the termination penalty as a reward
            pen = float(np.float32(M.SortingEnvConfig().overflow_termination_penalty))
            assert int((got["rewards"] == pen).sum()) >= 1, "no episode ended by overflow"
        a.close()
        d.close()


# ---- 2. the twin's labels with a sorting policy (the fused collector refuses that pair by name) -------------------------------
def test_the_twin_labels_with_a_sort_policy_and_the_fused_collector_refuses_it():
    import torch

    import marl_sortingenv_amd as M

    pol, sorter = _actor("press"), _actor("sort")
    a, d = _env("press", 33), _env("press", 33)
    tw = M.PolicyRolloutCollector(a, pol, 7, sort_policy=sorter, seed=SEED, expert_labels=True).collect()
    out = None
    for k in range(7):  # the hand loop: the label before the step, the sorting agent's decision stepped with the action
        assert torch.equal(tw["expert_actions"][k], d.rule_actions()), k
        out = sorter.forward(d.sort_agent_obs(), None, deterministic=True, out=out)
        d.step(tw["actions"][k], sort_mode=out["action"])
    _state_equal("twin with sort_policy", a, d)
    with pytest.raises(ValueError, match="PolicyRolloutCollector"):
        M.FusedPolicyRollout(a, pol, 7, sort_policy=sorter, expert_labels=True)
    a.close()
    d.close()


# ---- 3. memory and refusals ---------------------------------------------------------------------------------------------------
OUTS = NINE[:7] + ("last_values", "last_dones", "expert_actions")


def _sizes(kind, n, K):
    D, A = DIMS[kind]
    sizes = {"observations": K * n * D * 4, "action_masks": K * n * A, "actions": K * n * 4, "log_probs": K * n * 4,
             "values": K * n * 4, "rewards": K * n * 4, "episode_starts": K * n, "last_values": n * 4, "last_dones": n,
             "expert_actions": K * n * 4}
    assert tuple(sizes) == OUTS
    return sizes


def _raw_call(env, pol, K, flags, ptrs, seed=SEED, det=0, sort_mode=None):
    import torch

    L = env.L if env is not None else pol.L
    p = [None if ptrs.get(name) is None else C.c_void_p(ptrs[name]) for name in OUTS]
    return L.mse_rollout_policy_labelled(None if env is None else env._h, None if pol is None else pol._h, K, seed, det, sort_mode,
                                         flags, *p, C.c_void_p(torch.cuda.current_stream().cuda_stream))


def _check_call(env, pol, K, flags=0, seed=SEED, det=0):
    L = env.L if env is not None else pol.L
    return L.mse_rollout_policy_labelled_check(None if env is None else env._h, None if pol is None else pol._h, K, seed, det, None, flags)


@pytest.mark.parametrize("kind", ["sort", "mono"])
def test_labelled_rollout_memory(kind):
    """97 envs (a ragged wave): no guard byte is written, and each optional output may be NULL in turn with the others
    unchanged"""
    import torch

    n, K = 97, 4
    pol = _actor(kind)
    env = _env(kind, n)
    raw, at = guarded(_sizes(kind, n, K))
    ptrs = {name: raw.data_ptr() + off for name, (off, _) in at.items()}
    assert _raw_call(env, pol, K, 0, ptrs) == 0
    torch.cuda.synchronize()
    within = inside(raw, at)
    assert bool((raw[~within] == 0xA5).all()), "a guard byte was written"
    full = raw.clone()
    for name in NINE:  # each optional output NULL in turn
        e2 = _env(kind, n)
        raw.fill_(0xA5)
        assert _raw_call(e2, pol, K, 0, dict(ptrs, **{name: None})) == 0
        torch.cuda.synchronize()
        off, size = at[name]
        assert bool((raw[off:off + size] == 0xA5).all()), name
        keep = within.clone()
        keep[off:off + size] = False
        assert torch.equal(raw[keep], full[keep]) and bool((raw[~within] == 0xA5).all()), name
        _state_equal(f"{name} NULL", env, e2)
        e2.close()
    env.close()


def test_labelled_rollout_refusals():
    import torch

    import marl_sortingenv_amd as M

    INVALID, UNSUPPORTED, ALIGNMENT, NOT_RESET = -1, -2, -6, None
    kind, n, K = "mono", 64, 2
    pol = _actor(kind)
    opened = []

    def keep(e):
        opened.append(e)
        return e

    try:
        env = keep(_env(kind, n))
        raw, at = guarded(_sizes(kind, n, K))
        ptrs = {name: raw.data_ptr() + off for name, (off, _) in at.items()}
        assert _check_call(env, pol, K) == 0 and env.policy_step == 0  # the check launches nothing
        assert _raw_call(env, pol, K, 0, ptrs) == 0
        torch.cuda.synchronize()
        filled, state, t = raw.clone(), [x.clone() for x in env.get_state()], env.policy_step

        def refused(status, e=env, a=pol, k=K, flags=0, p=None, check_too=True):
            """The check-only entry first (same status, same message), then the entry that could launch; status None: any refusal"""
            msg = None
            if check_too:
                rc = _check_call(e, a, k, flags)
                assert rc == status if status is not None else rc < 0
                msg = pol.L.mse_last_error()
            before = None if e is None else e.policy_step
            rc = _raw_call(e, a, k, flags, ptrs if p is None else p)
            assert rc == status if status is not None else rc < 0
            assert msg is None or pol.L.mse_last_error() == msg
            torch.cuda.synchronize()
            assert torch.equal(raw, filled), "a refused call wrote to the buffers"
            assert before is None or e.policy_step == before

        refused(INVALID, e=None)
        refused(INVALID, a=None)
        refused(INVALID, k=0)
        refused(INVALID, k=-1)
        refused(INVALID, a=_actor("press"))
        refused(INVALID, a=_actor("sort"))
        for flag in (4, 8, 16, 32, 64, 128, 256, 512, 1024, 1 << 31):  # every bit that is not one of the two
            refused(INVALID, flags=flag)
        assert _check_call(env, pol, K, flags=1 | 2) == 0
        refused(INVALID, e=keep(_env(kind, n, auto_reset=False)))
        refused(NOT_RESET, e=keep(_env(kind, n, reset_now=False)))
        env.trace_begin(0, 16)
        refused(INVALID)
        env.trace_end()
        for name in ("observations", "action_masks"):  # the 16-byte rule
            refused(ALIGNMENT, p=dict(ptrs, **{name: ptrs[name] + 4}), check_too=False)
        refused(INVALID, p=dict(ptrs, expert_actions=None), check_too=False)
        assert b"expert_actions_out is NULL" in pol.L.mse_last_error()
        cfg = M.SortingEnvConfig()
        refused(UNSUPPORTED, e=keep(_env(kind, n, literal_choice=True)))
        refused(UNSUPPORTED, e=keep(_env(kind, n, config=cfg.with_overrides(GEN))))
        # tables that do not fit: the same config is served in 32-env waves and refused in 64-env waves
        big_cfg = cfg.with_overrides(BIG_TABLES)
        small_big = keep(_env(kind, n, config=big_cfg))
        assert _check_call(small_big, pol, K) == 0 and _raw_call(small_big, pol, K, 0, ptrs) == 0
        torch.cuda.synchronize()
        filled = raw.clone()
        big = keep(_env(kind, 256 * cus() + 1, config=big_cfg))
        refused(UNSUPPORTED, e=big)
        assert b"LDS image does not fit" in pol.L.mse_last_error() and big.policy_step == 0
        with pytest.raises(M.MseError):
            M.FusedPolicyRollout(big, pol, K, expert_labels=True).collect()
        # the env the refusals were tried on is where it was, and still serves
        for x, y in zip(state, env.get_state()):
            assert torch.equal(x, y)
        assert env.policy_step == t
        assert M.FusedPolicyRollout(env, pol, K, expert_labels=True).collect()["expert_actions"].shape == (K, n)
    finally:
        for e in opened:
            e.close()


# ---- 4. the learner ---------------------------------------------------------------------------------------------------------------
def test_learn_on_the_fused_labelled_collector_is_learn_on_the_twin():
    import torch

    import marl_sortingenv_amd as M

    runs = []
    for fused in (True, False):
        pol = M.MlpPolicy.random_init(29, 22, seed=31)
        env = _env("mono", 96, max_steps=12, base_seed=21)
        col = (M.FusedPolicyRollout if fused else M.PolicyRolloutCollector)(env, pol, 8, seed=22, expert_labels=True)
        learner = M.PPOLearner(pol, learning_rate=1e-3, n_epochs=2, batch_size=256, seed=5, ent_coef=0.05, bc_coef=1.0)
        runs.append((learner.learn(col, 2), learner.weights.clone(), env))
    (rec_a, w_a, env_a), (rec_b, w_b, env_b) = runs
    assert rec_a == rec_b and torch.equal(w_a.view(torch.int32), w_b.view(torch.int32))
    assert rec_a[0]["bc_coef"] == 1.0 and rec_a[0]["bc_loss"] > 0.0
    for name, x, y in zip(("ints", "dbls", "rng"), env_a.get_state(), env_b.get_state()):
        assert torch.equal(x, y), name
