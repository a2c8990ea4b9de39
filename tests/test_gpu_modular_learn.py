"""GPU: training the modular pair on what FusedModularRollout collects - each agent's view of the rollout under
PPOLearner's names, GAE on that agent's reward, and ModularTrainer (one collect, one update per learner, a frozen agent
without one).  N = 256, K = 8.  Episodes last 36 steps and every test starts 32 steps into them: press_action_masks()
leaves the pressing agent a choice there (in the first steps of an episode only action 0 is legal), and every env ends
an episode inside the next rollout."""
import numpy as np
import pytest

from tests import ppo_reference as R

pytestmark = pytest.mark.gpu

N, K = 256, 8
MAX_STEPS, PRE_ROLLS = 36, 4


def _setup(seed=0, press_masked=True, base_seed=3):
    import marl_sortingenv_amd as M

    env = M.BatchedSortingEnv(kind="mono", num_envs=N, device=0, base_seed=base_seed, max_steps=MAX_STEPS, noise_sorting=0.05,
                              balesize=200)
    sort_ag = M.MlpPolicy.random_init(13, 2, seed=seed + 1, precision="f16x3")
    press_ag = M.MlpPolicy.random_init(16, 11, seed=seed + 2, precision="f16x3")
    col = M.FusedModularRollout(env, sort_ag, press_ag, K, press_masked=press_masked)
    for _ in range(PRE_ROLLS):
        col.collect()
    return env, sort_ag, press_ag, col


def _learner(policy, seed):
    import marl_sortingenv_amd as M

    return M.PPOLearner(policy, n_epochs=2, batch_size=512, ent_coef=0.05, seed=seed)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("reward", ["own", "team"])
def test_gae_on_each_view(reward):
    import marl_sortingenv_amd as M

    env, _, _, col = _setup()
    b = col.collect()
    assert b["episode_starts"][1:].cpu().numpy().any(axis=0).all(), "every env ends an episode inside the rollout"
    assert float((b["press_masks"].sum(dim=2) > 1).float().mean()) > 0.05, "the masks leave the presser no choice"
    for who in ("sort", "press"):
        v = col.view(who, reward)
        rkey = "rewards" if reward == "team" else f"rewards_{who}"
        assert v["rewards"] is b[rkey] and v["observations"] is b[f"{who}_obs"] and v["values"] is b[f"{who}_values"]
        assert v["last_values"] is b[f"{who}_last_values"] and v["episode_starts"] is b["episode_starts"]
        assert (v["action_masks"] is b["press_masks"]) if who == "press" else (v["action_masks"] is None)
        M.compute_gae(v, 0.99, 0.95)
        ea, er = R.gae_numpy(*(b[k].cpu().numpy() for k in (rkey, f"{who}_values", "episode_starts", f"{who}_last_values",
                                                            "last_dones")), 0.99, 0.95)
        assert np.array_equal(_bits(v["advantages"]), ea.view(np.uint32)), (who, reward)
        assert np.array_equal(_bits(v["returns"]), er.view(np.uint32)), (who, reward)
        assert col.view(who, reward) is v  # the view is kept, with its advantages and returns
    # the parts add up to the team reward (f64 sum rounded once against two f32 roundings: within an ulp of the sum)
    total = b["rewards_sort"].double() + b["rewards_press"].double()
    assert float((total - b["rewards"].double()).abs().max()) <= 2.0 ** -22 * float(b["rewards"].abs().max())
    env.close()


def test_unmasked_presser_view_has_no_masks():
    env, _, _, col = _setup(press_masked=False)
    col.collect()
    assert col.view("press")["action_masks"] is None and col.view("sort")["action_masks"] is None
    env.close()


@pytest.mark.parametrize("reward", ["own", "team"])
def test_trainer_equals_hand_loop(reward):
    import marl_sortingenv_amd as M

    runs = []
    for by_hand in (False, True):
        env, sort_ag, press_ag, col = _setup()
        ls, lp = _learner(sort_ag, 5), _learner(press_ag, 6)
        if by_hand:
            recs = []
            for it in range(3):
                data = col.collect()
                rec = {"reward": float(data["rewards"].mean()), "reward_sort": float(data["rewards_sort"].mean()),
                       "reward_press": float(data["rewards_press"].mean())}
                p = 1.0 - (it + 1) / 3
                rec["sort"] = ls.update(col.view("sort", reward), progress_remaining=p)["mean"]
                rec["press"] = lp.update(col.view("press", reward), progress_remaining=p)["mean"]
                recs.append(rec)
        else:
            recs = M.ModularTrainer(col, ls, lp, reward=reward).learn(3)
        runs.append((recs, ls.weights.clone(), lp.weights.clone(), sort_ag.flat_weights().copy(), press_ag.flat_weights().copy()))
        env.close()
    (ra, sa, pa, fsa, fpa), (rb, sb, pb, fsb, fpb) = runs
    assert ra == rb
    assert np.array_equal(_bits(sa), _bits(sb)) and np.array_equal(_bits(pa), _bits(pb))
    assert np.array_equal(fsa.view(np.uint32), fsb.view(np.uint32)) and np.array_equal(fpa.view(np.uint32), fpb.view(np.uint32))
    assert set(ra[0]) == {"sort", "press", "reward", "reward_sort", "reward_press"}
    w0 = M.MlpPolicy.random_init(13, 2, seed=1, precision="f16x3").flat_weights()
    assert not np.array_equal(w0, fsa), "the sorter did not learn"


def test_trainer_records_episodes_and_evaluations():
    import math

    import marl_sortingenv_amd as M

    env, sort_ag, press_ag, col = _setup()
    eval_env = M.BatchedSortingEnv(kind="mono", num_envs=8, device=0, base_seed=900, max_steps=5, noise_sorting=0.05, balesize=200)
    seen = []
    recs = M.ModularTrainer(col, _learner(sort_ag, 5), _learner(press_ag, 6)).learn(
        2, callback=lambda it, rec: seen.append(it), episode_stats=True, eval_env=eval_env, eval_freq=2, n_eval_episodes=8)
    assert seen == [0, 1] and len(recs) == 2
    # the account starts with the trainer, 32 steps into every env's episode: each ends once, 4 steps later
    assert recs[0]["episodes"] == N and recs[0]["ep_len_mean"] == float(MAX_STEPS - PRE_ROLLS * K)
    assert math.isfinite(recs[0]["ep_rew_mean"]) and recs[1]["episodes"] == 0
    assert "eval_mean_reward" not in recs[0] and math.isfinite(recs[1]["eval_mean_reward"]) and recs[1]["eval_std_reward"] >= 0.0
    want = M.evaluate_rollout(eval_env, "model", n_eval_episodes=8, sort_agent=sort_ag, press_agent=press_ag, press_agent_maskable=True)
    assert (recs[1]["eval_mean_reward"], recs[1]["eval_std_reward"]) == want
    env.close()
    eval_env.close()


def test_trainer_with_a_frozen_sorter():
    import torch

    import marl_sortingenv_amd as M

    env, sort_ag, press_ag, col = _setup()
    w_before = sort_ag.flat_weights().copy()
    image = torch.empty(int(sort_ag.L.mse_policy_image_floats()), dtype=torch.float32)
    import ctypes as C

    def read_image():
        assert sort_ag.L.mse_policy_read_image(sort_ag._h, C.c_void_p(image.data_ptr())) == 0
        return image.clone()

    image_before = read_image()
    press_w0 = press_ag.flat_weights().copy()
    choices = []
    recs = M.ModularTrainer(col, press_learner=_learner(press_ag, 6)).learn(
        2, callback=lambda it, rec: choices.append(len(torch.unique(col.buffers["press_actions"]))))
    assert all("sort" not in r and "press" in r for r in recs)
    assert np.array_equal(sort_ag.flat_weights().view(np.uint32), w_before.view(np.uint32))
    assert torch.equal(read_image().view(torch.int32), image_before.view(torch.int32))
    assert not np.array_equal(press_ag.flat_weights(), press_w0)
    # the frozen agent's recorded actions are its argmax on the recorded rows
    b = col.buffers
    det = sort_ag.forward(b["sort_obs"].reshape(-1, 13), None, deterministic=True)["action"]
    assert torch.equal(det, b["sort_actions"].reshape(-1))
    assert max(choices) > 1, "the presser never had a choice"
    env.close()


def test_trainer_refusals():
    import marl_sortingenv_amd as M

    env, sort_ag, press_ag, col = _setup()
    with pytest.raises(ValueError, match="at least one learner"):
        M.ModularTrainer(col)
    foreign = M.MlpPolicy.random_init(13, 2, seed=77, precision="f16x3")
    with pytest.raises(ValueError, match="sort_agent"):
        M.ModularTrainer(col, sort_learner=_learner(foreign, 1))
    with pytest.raises(ValueError, match="press_agent"):
        M.ModularTrainer(col, press_learner=_learner(M.MlpPolicy.random_init(16, 11, seed=78, precision="f16x3"), 1))
    with pytest.raises(ValueError, match="reward"):
        M.ModularTrainer(col, sort_learner=_learner(sort_ag, 1), reward="mine")
    with pytest.raises(ValueError):
        col.view("sorter")
    with pytest.raises(ValueError):
        col.view("sort", reward="theirs")
    with pytest.raises(ValueError, match="first_iteration"):
        M.ModularTrainer(col, sort_learner=_learner(sort_ag, 1)).learn(2, first_iteration=3)
    env.close()


def test_collector_state_dict_resumes_bit_for_bit():
    import torch

    import marl_sortingenv_amd as M

    env, sort_ag, press_ag, col = _setup()
    col.collect()
    sd = col.state_dict()
    assert sd["collector"] == "modular" and sd["sort_seed"] == 2024 and sd["press_seed"] == 2025 and sd["n_steps"] == K
    want = {k: v.clone() for k, v in col.collect().items()}
    env2 = M.BatchedSortingEnv(kind="mono", num_envs=N, device=0, base_seed=3, max_steps=MAX_STEPS, noise_sorting=0.05, balesize=200)
    col2 = M.FusedModularRollout(env2, sort_ag, press_ag, K)
    col2.load_state_dict(sd)
    got = col2.collect()
    for k in want:
        assert torch.equal(got[k], want[k]), k
    with pytest.raises(ValueError):
        M.FusedModularRollout(env2, sort_ag, press_ag, K, press_seed=99).check_state_dict(sd)
    with pytest.raises(ValueError):
        M.FusedModularRollout(env2, sort_ag, press_ag, K + 1).check_state_dict(sd)
    env.close()
    env2.close()
