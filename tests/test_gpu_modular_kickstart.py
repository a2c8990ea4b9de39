"""GPU: the rule-based controller teaching the modular pair inside ModularTrainer, on a labelled FusedModularRollout -
PPOLearner(bc_coef=...) on view(), ImitationLearner on demo_view() with a beta schedule, one of each, a frozen agent, and the
checkpoint round trip of the labelled collector.  Every loop is held against the same loop written out by hand, on bits;
no learning outcome is asserted.  N = 256, K = 8, 36-step episodes entered 32 steps in (tests/test_gpu_modular_learn.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, K = 256, 8
MAX_STEPS, PRE_ROLLS = 36, 4
ITERATIONS = 3


def _beta(fraction):
    return 1.0 - fraction


def _setup(gamma=None, seed=0):
    import marl_sortingenv_amd as M

    env = M.BatchedSortingEnv(kind="mono", num_envs=N, device=0, base_seed=3, max_steps=MAX_STEPS, noise_sorting=0.05, balesize=200)
    sort_ag = M.MlpPolicy.random_init(13, 2, seed=seed + 1, precision="f16x3")
    press_ag = M.MlpPolicy.random_init(16, 11, seed=seed + 2, precision="f16x3")
    col = M.FusedModularRollout(env, sort_ag, press_ag, K, expert_labels=True, gamma=gamma)
    for _ in range(PRE_ROLLS):
        col.collect()
    return env, sort_ag, press_ag, col


def _ppo(policy, seed):
    import marl_sortingenv_amd as M

    return M.PPOLearner(policy, n_epochs=2, batch_size=512, ent_coef=0.05, seed=seed, bc_coef=lambda p: 0.5 * p)


def _il(policy, seed):
    import marl_sortingenv_amd as M

    return M.ImitationLearner(policy, n_epochs=2, batch_size=512, seed=seed)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _hand_loop(col, learners, reward, beta):
    import marl_sortingenv_amd as M

    recs = []
    for it in range(ITERATIONS):
        if beta is not None:
            col.beta = float(beta(it / ITERATIONS) if callable(beta) else beta)
        data = col.collect(sort_deterministic=learners["sort"] is None, press_deterministic=learners["press"] is None)
        rec = {"reward": float(data["rewards"].mean()), "reward_sort": float(data["rewards_sort"].mean()),
               "reward_press": float(data["rewards_press"].mean())}
        if beta is not None:
            rec.update(beta=col.beta, expert_share=float(data["expert_stepped"].float().mean()))
        for who in ("sort", "press"):
            learner = learners[who]
            if isinstance(learner, M.ImitationLearner):
                rec[who] = learner.update(col.demo_view(who))["mean"]
            elif learner is not None:
                rec[who] = learner.update(col.view(who, reward), progress_remaining=1.0 - (it + 1) / ITERATIONS)["mean"]
        recs.append(rec)
    return recs


def _both_ways(make_learners, reward="own", beta=None, gamma=None):
    """-> the trainer's records, after checking them and both agents' weights against the hand loop on bits."""
    import marl_sortingenv_amd as M

    runs = []
    for by_hand in (False, True):
        env, sort_ag, press_ag, col = _setup(gamma)
        learners = make_learners(sort_ag, press_ag)
        if by_hand:
            recs = _hand_loop(col, learners, reward, beta)
        else:
            recs = M.ModularTrainer(col, learners["sort"], learners["press"], reward=reward).learn(ITERATIONS, beta=beta)
        runs.append((recs, sort_ag.flat_weights().copy(), press_ag.flat_weights().copy(),
                     [None if l is None else l.weights.clone() for l in learners.values()], [x.clone() for x in env.get_state()]))
        env.close()
    (ra, sa, pa, la, ea), (rb, sb, pb, lb, eb) = runs
    assert ra == rb
    assert np.array_equal(sa.view(np.uint32), sb.view(np.uint32)) and np.array_equal(pa.view(np.uint32), pb.view(np.uint32))
    for x, y in zip(la, lb):
        assert (x is None and y is None) or np.array_equal(_bits(x), _bits(y))
    for x, y in zip(ea, eb):
        assert np.array_equal(x.cpu().numpy(), y.cpu().numpy())
    return ra, sa, pa


def _fresh(obs_dim, n_actions, seed):
    import marl_sortingenv_amd as M

    return M.MlpPolicy.random_init(obs_dim, n_actions, seed=seed, precision="f16x3").flat_weights()


@pytest.mark.parametrize("reward", ["own", "team"])
def test_two_ppo_learners_with_an_imitation_term(reward):
    recs, sw, pw = _both_ways(lambda s, p: {"sort": _ppo(s, 5), "press": _ppo(p, 6)}, reward=reward)
    assert set(recs[0]) == {"sort", "press", "reward", "reward_sort", "reward_press"}
    for who in ("sort", "press"):
        assert {"bc_loss", "bc_accuracy", "bc_unusable"} <= set(recs[0][who])
        assert all(np.isfinite(r[who]["bc_loss"]) for r in recs)
    assert not np.array_equal(_fresh(13, 2, 1), sw) and not np.array_equal(_fresh(16, 11, 2), pw)


def test_two_imitation_learners_with_a_beta_schedule():
    recs, sw, pw = _both_ways(lambda s, p: {"sort": _il(s, 5), "press": _il(p, 6)}, beta=_beta, gamma=0.99)
    assert [r["beta"] for r in recs] == [float(_beta(it / ITERATIONS)) for it in range(ITERATIONS)]
    assert recs[0]["expert_share"] == 1.0 and all(0.0 < r["expert_share"] < 1.0 for r in recs[1:])
    for who in ("sort", "press"):
        assert {"bc_loss", "accuracy", "unusable", "value_loss"} <= set(recs[0][who])
    assert recs[0]["sort"]["unusable"] == 0.0  # the sorter has no mask
    assert not np.array_equal(_fresh(13, 2, 1), sw) and not np.array_equal(_fresh(16, 11, 2), pw)


def test_one_learner_of_each_kind():
    """The sorter cloned, the presser on PPO with the imitation term: allowed at beta = 0, where every row is the pair's own."""
    recs, _, _ = _both_ways(lambda s, p: {"sort": _il(s, 5), "press": _ppo(p, 6)}, beta=0.0)
    assert "accuracy" in recs[0]["sort"] and "bc_accuracy" in recs[0]["press"]
    assert all(r["beta"] == 0.0 and r["expert_share"] == 0.0 for r in recs)


def test_a_frozen_agent_keeps_its_weights():
    recs, sw, pw = _both_ways(lambda s, p: {"sort": None, "press": _il(p, 6)}, beta=0.5)
    assert "sort" not in recs[0] and np.array_equal(_fresh(13, 2, 1).view(np.uint32), sw.view(np.uint32))
    assert not np.array_equal(_fresh(16, 11, 2), pw)


def test_trainer_refusals():
    import marl_sortingenv_amd as M

    env, sort_ag, press_ag, col = _setup()
    before = press_ag.flat_weights().copy()
    with pytest.raises(ValueError, match="on-policy|own"):
        M.ModularTrainer(col, _il(sort_ag, 5), _ppo(press_ag, 6)).learn(2, beta=0.5)
    with pytest.raises(ValueError):
        M.ModularTrainer(col, _ppo(sort_ag, 5), _ppo(press_ag, 6)).learn(2, beta=_beta)
    assert np.array_equal(before, press_ag.flat_weights())
    # the collector's own beta, with none passed to learn(): refused alike, before anything is collected
    col.beta, t0 = 0.5, env.policy_step
    with pytest.raises(ValueError, match="on-policy|own"):
        M.ModularTrainer(col, _il(sort_ag, 5), _ppo(press_ag, 6)).learn(2)
    assert env.policy_step == t0 and np.array_equal(before, press_ag.flat_weights())
    col.beta = 0.0
    plain = M.FusedModularRollout(env, sort_ag, press_ag, K)
    with pytest.raises(ValueError, match="expert_labels"):
        M.ModularTrainer(plain, _il(sort_ag, 5))
    with pytest.raises(ValueError, match="expert_labels"):
        M.ModularTrainer(plain, M.PPOLearner(sort_ag, n_epochs=1)).learn(1, beta=0.0)
    env.close()


@pytest.mark.parametrize("twin", [False, True], ids=["fused", "twin"])
def test_checkpoint_round_trip_of_a_labelled_collector(twin, tmp_path):
    """2 collections, checkpoint, load into fresh objects, 2 more: the rows of 4 collections run straight through - the
    label keys among them, with the beta the file carries."""
    import torch

    import marl_sortingenv_amd as M

    cls = M.ModularRolloutCollector if twin else M.FusedModularRollout
    keys = ("sort_obs", "press_obs", "press_masks", "episode_starts", "sort_actions", "press_actions", "rewards", "sort_expert_actions",
            "press_expert_actions", "stepped_actions", "expert_stepped", "returns", "last_dones")
    n = 64

    def make(beta):
        env = M.BatchedSortingEnv(kind="mono", num_envs=n, device=0, base_seed=3, max_steps=5, noise_sorting=0.05, balesize=200)
        sort_ag = M.MlpPolicy.random_init(13, 2, seed=1, precision="f16x3")
        press_ag = M.MlpPolicy.random_init(16, 11, seed=2, precision="f16x3")
        return env, cls(env, sort_ag, press_ag, K, expert_labels=True, beta=beta, mix_seed=77, gamma=0.99)

    env, col = make(0.25)
    straight = []
    for _ in range(4):
        b = col.collect()
        straight.append({k: b[k].clone() for k in keys})
    env.close()
    env, col = make(0.25)
    for _ in range(2):
        col.collect()
    path = M.save_checkpoint(tmp_path / "run.pt", collector=col, iteration=2)
    env.close()
    env, col = make(0.0)  # the mixture comes from the file
    M.load_checkpoint(path, collector=col)
    assert col.beta == 0.25
    for want in straight[2:]:
        got = col.collect()
        for k in keys:
            assert torch.equal(got[k].view(torch.uint8), want[k].view(torch.uint8)), k
    other_env, other = make(0.25)
    other.mix_seed = 78
    with pytest.raises(ValueError, match="mix_seed"):
        M.load_checkpoint(path, collector=other)
    env.close()
    other_env.close()
