"""GPU: the learners on the preview view (FusedPolicyRollout(view="preview"), FusedDemonstrationRollout(agent="preview")).
The row names are the own view's, so PPOLearner.learn, PPOLearner(bc_coef=...), ImitationLearner.learn(beta=...) and
evaluate_policy run unchanged; each is held against the same loop over the multi-launch twin, on bits, at N = 64, K = 8.
Then the collector's checkpoint surface (the key `view`) and every constructor refusal."""
import numpy as np
import pytest

from tests.rollout_checks import bits_equal, who_host
from tests.test_gpu_demo_rollout import _actor
from tests.test_gpu_preview_rollout import MIX_SEED, SEED, _env

pytestmark = pytest.mark.gpu

N, K = 64, 8


def _same_run(a, b):
    import torch

    (rec_a, w_a, env_a), (rec_b, w_b, env_b) = a, b
    assert rec_a == rec_b, "the records differ"
    assert torch.equal(w_a.view(torch.int32), w_b.view(torch.int32)), "the weights differ"
    for name, x, y in zip(("ints", "dbls", "rng"), env_a.get_state(), env_b.get_state()):
        assert torch.equal(x, y), name
    assert env_a.policy_step == env_b.policy_step


@pytest.mark.parametrize("bc", [False, True], ids=["ppo", "ppo_bc"])
def test_ppo_on_the_fused_preview_collector_is_ppo_on_the_twin(bc):
    import marl_sortingenv_amd as M

    runs = []
    for fused in (True, False):
        pol = M.MlpPolicy.random_init(29, 22, seed=31)
        env = _env(N, max_steps=12, base_seed=21)
        col = (M.FusedPolicyRollout if fused else M.PolicyRolloutCollector)(env, pol, K, seed=22, view="preview", expert_labels=bc)
        assert ("expert_actions" in col.buffers) == bc
        learner = M.PPOLearner(pol, learning_rate=1e-3, n_epochs=2, batch_size=256, seed=5, ent_coef=0.05,
                               bc_coef=1.0 if bc else None)
        runs.append((learner.learn(col, 2), learner.weights.clone(), env))
    _same_run(*runs)
    rec = runs[0][0]
    assert len(rec) == 2 and (rec[0]["bc_coef"] == 1.0 and rec[0]["bc_loss"] > 0.0 if bc else "bc_loss" not in rec[0])
    # the preview is another row than the own view's: the same run on view="own" trains on other observations
    pol = M.MlpPolicy.random_init(29, 22, seed=31)
    envs = [_env(N, max_steps=12, base_seed=21) for _ in range(2)]
    own = M.FusedPolicyRollout(envs[0], pol, K, seed=22).collect()
    pre = M.FusedPolicyRollout(envs[1], pol, K, seed=22, view="preview").collect()
    assert own["observations"].shape == pre["observations"].shape and not bool((own["observations"] == pre["observations"]).all())
    for env in envs + [run[2] for run in runs]:
        env.close()


class _HandPreviewDemo:
    """DemonstrationCollector(agent="preview", actor=student) with the who-steps rule of the header between the student's
    action and the step: what FusedDemonstrationRollout(agent="preview") does in one launch, written out over the
    multi-launch collector's own view, buffers and returns."""

    def __init__(self, env, n_steps, actor, gamma):
        import marl_sortingenv_amd as M

        self.inner = M.DemonstrationCollector(env, n_steps, agent="preview", actor=actor, gamma=gamma, seed=SEED)
        self.env, self.actor, self.beta = env, actor, 1.0

    def collect(self):
        import torch

        import marl_sortingenv_amd as M
        from marl_sortingenv_amd._lib import check
        from marl_sortingenv_amd.learner import _ptr, _stream

        c, env = self.inner, self.env
        b, n_steps = c.buffers, c.n_steps
        threshold = M.expert_threshold(self.beta)
        stepped_by = torch.empty((n_steps, env.num_envs), dtype=torch.uint8, device=env.device)
        for k in range(n_steps):
            t = env.policy_step
            obs, mask = c._view()
            rule = env.rule_actions()
            a = self.actor.forward(obs, mask, seed=SEED, t=t, index_offset=env.index_offset)["action"]
            who = torch.from_numpy(who_host(env, MIX_SEED, t, threshold)).to(env.device)
            b["observations"][k].copy_(obs)
            b["action_masks"][k].copy_(mask)
            b["episode_starts"][k].copy_(c._last_done)
            b["actions"][k].copy_(rule)
            b["stepped_actions"][k].copy_(torch.where(who != 0, rule, a))
            stepped_by[k].copy_(who)
            _, rew, done, _ = env.step(b["stepped_actions"][k])
            b["rewards"][k].copy_(rew)
            c._last_done.copy_(done)
        last_dones = c._last_done.clone()
        with torch.cuda.device(env.device):
            check(env.L.mse_gae(n_steps, env.num_envs, _ptr(b["rewards"]), _ptr(c._zeros), _ptr(b["episode_starts"]),
                                _ptr(c._zeros[n_steps]), _ptr(last_dones), c.gamma, 1.0, _ptr(c._adv), _ptr(b["returns"]),
                                _stream(env.device)))
        return dict(b, last_dones=last_dones, expert_stepped=stepped_by)


def test_imitation_with_a_beta_schedule_is_the_hand_loop():
    """ImitationLearner.learn(beta=lambda d: 1 - d) for two iterations: beta 1, then 0.5."""
    import torch

    import marl_sortingenv_amd as M

    runs, shares = [], []
    for which in ("fused", "hand"):
        pol = M.MlpPolicy.random_init(29, 22, seed=71)
        env = _env(N, max_steps=5)
        if which == "fused":
            col = M.FusedDemonstrationRollout(env, K, actor=pol, gamma=0.97, seed=SEED, mix_seed=MIX_SEED, agent="preview")
            assert col.beta == 0.0
        else:
            col = _HandPreviewDemo(env, K, pol, 0.97)
        learner = M.ImitationLearner(pol, learning_rate=1e-3, n_epochs=2, batch_size=100, seed=5)
        hist = learner.learn(col, 2, beta=lambda d: 1.0 - d)
        torch.cuda.synchronize()
        runs.append((hist, learner.weights.clone(), env))
        shares.append([r["expert_share"] for r in hist])
    _same_run(*runs)
    hist = runs[0][0]
    assert [r["beta"] for r in hist] == [1.0, 0.5] and hist[0]["expert_share"] == 1.0 and 0.35 < hist[1]["expert_share"] < 0.65
    assert 0.0 < hist[0]["accuracy"] <= 1.0
    for _, _, env in runs:
        env.close()


@pytest.mark.parametrize("beta", [0.0, 1.0])
def test_fused_preview_demo_at_the_ends_is_the_demonstration_collector(beta):
    """beta = 0: DemonstrationCollector(agent="preview", actor=student); beta = 1: what actor=None steps.  The same dict."""
    import marl_sortingenv_amd as M

    pol = _actor("mono")
    a, b = _env(N), _env(N)
    fused = M.FusedDemonstrationRollout(a, K, actor=pol, beta=beta, gamma=0.97, seed=SEED, mix_seed=MIX_SEED, agent="preview")
    twin = M.DemonstrationCollector(b, K, agent="preview", actor=pol if beta == 0.0 else None, gamma=0.97, seed=SEED)
    for launch in range(2):
        got, exp = fused.collect(), twin.collect()
        assert set(got) == set(exp) | {"expert_stepped"}
        bits_equal(f"beta={beta} launch {launch}", got, exp, tuple(exp))
        assert bool((got["expert_stepped"] == int(beta)).all())
        assert got["observations"].shape == (K, N, 29) and got["action_masks"].shape == (K, N, 22)
        for x, y in zip(a.get_state(), b.get_state()):
            assert bool((x == y).all())
    a.close()
    b.close()


class _MonoAgent:
    """A stored mono_agent over an MlpPolicy: predict() is one deterministic forward on the row it is handed."""

    def __init__(self, pol):
        self.pol, self.calls = pol, 0

    def predict(self, obs, deterministic=True, action_masks=None):
        import torch

        assert deterministic is True and action_masks is not None
        self.calls += 1
        o = torch.from_numpy(np.asarray(obs, dtype=np.float32))[None].cuda()
        m = torch.from_numpy(np.asarray(action_masks).astype(np.uint8))[None].cuda()
        return int(self.pol.forward(o, m, deterministic=True)["action"][0].item()), None


def test_evaluate_policy_on_the_preview_view_is_env3_with_a_stored_mono_agent():
    """Three seeds, one episode of 12 steps each: the deterministic fused preview collector under evaluate_policy against
    Env_3_Monolith.step() with set_agents(mono_agent=...) over the same weights.  The lengths are equal; a return is the
    sum of at most 12 float32 rewards there and of the float64 rewards here, each within 2^-24 |r| (|r| <= 10) of the other:
    1e-5 bounds the difference."""
    import marl_sortingenv_amd as M

    base, max_steps = 300, 12
    pol = _actor("mono")
    env = _env(3, max_steps=max_steps, base_seed=base)
    col = M.FusedPolicyRollout(env, pol, max_steps, seed=SEED, view="preview")
    returns, lengths = M.evaluate_policy(col, 3, deterministic=True, return_episode_rewards=True)
    want_r, want_l = [], []
    agent = _MonoAgent(pol)
    for i in range(3):
        one = M.Env_3_Monolith(max_steps=max_steps, seed=base + i, noise_sorting=0.05, balesize=200)
        one.set_agents(mono_agent=agent)
        one.reset(seed=base + i)
        total, steps, done = 0.0, 0, False
        while not done:
            _, r, done, _, _ = one.step()
            total, steps = total + r, steps + 1
        want_r.append(total)
        want_l.append(steps)
        one.close()
    assert agent.calls == sum(want_l)
    assert sorted(int(x) for x in lengths) == sorted(want_l)
    assert np.abs(np.sort(np.asarray(returns, dtype=np.float64)) - np.sort(want_r)).max() <= 1e-5, (returns, want_r)
    env.close()


def test_checkpoint_round_trip_and_view_mismatch():
    import marl_sortingenv_amd as M

    pol = _actor("mono")
    for cls in (M.FusedPolicyRollout, M.PolicyRolloutCollector):
        a, b, c = _env(N), _env(N, base_seed=999), _env(N)
        one = cls(a, pol, K, seed=SEED, view="preview")
        one.collect()
        sd = one.state_dict()
        assert sd["view"] == "preview" and sd["collector"] == cls.KIND
        two = cls(b, pol, K, seed=SEED, view="preview")
        two.load_state_dict(sd)
        bits_equal(f"{cls.__name__} resumed", one.collect(), two.collect(),
                    ("observations", "action_masks", "actions", "log_probs", "values", "rewards", "episode_starts", "last_values",
                     "last_dones"))
        own = cls(c, pol, K, seed=SEED)
        own_sd = own.state_dict()
        assert "view" not in own_sd  # a checkpoint of the own view is what it was before there was a view
        own.check_state_dict(own_sd)
        with pytest.raises(ValueError, match=r"view mismatch.*'preview'.*'own'"):
            own.check_state_dict(sd)
        with pytest.raises(ValueError, match=r"view mismatch.*'own'.*'preview'"):
            two.load_state_dict(own_sd)
        for e in (a, b, c):
            e.close()


def test_constructor_refusals():
    import marl_sortingenv_amd as M

    pol, mono = _actor("mono"), _env(N)
    press = M.BatchedSortingEnv(kind="press", num_envs=N, device=0, auto_reset=True)
    for cls in (M.FusedPolicyRollout, M.PolicyRolloutCollector):
        with pytest.raises(ValueError, match="mono"):
            cls(press, _actor("press"), K, view="preview")
        with pytest.raises(ValueError, match="view must be"):
            cls(mono, pol, K, view="after")
        with pytest.raises(ValueError):
            cls(mono, _actor("press"), K, view="preview")
        assert cls(mono, pol, K).view == "own"
    col = M.FusedPolicyRollout(mono, pol, K, view="preview")
    t = mono.policy_step
    with pytest.raises(ValueError, match="use_action_masking"):
        col.collect(use_action_masking=False)
    assert mono.policy_step == t
    with pytest.raises(ValueError, match="mono"):
        M.DemonstrationCollector(press, K, agent="preview")
    with pytest.raises(ValueError, match="29 -> 22"):
        M.DemonstrationCollector(mono, K, agent="preview", actor=_actor("press"))
    with pytest.raises(ValueError, match=r"DemonstrationCollector\(agent='preview'\)"):
        M.FusedDemonstrationRollout(mono, K, agent="preview")
    with pytest.raises(ValueError, match="agent must be"):
        M.FusedDemonstrationRollout(mono, K, actor=pol, agent="sort")
    with pytest.raises(ValueError, match="mono"):
        M.FusedDemonstrationRollout(press, K, actor=_actor("press"), agent="preview")
    with pytest.raises(ValueError):
        M.FusedDemonstrationRollout(mono, K, actor=pol, agent="preview", seed=5, mix_seed=5)
    demo = M.FusedDemonstrationRollout(mono, K, actor=pol, agent="preview")
    for bad in (float("nan"), -0.1, 1.5):
        with pytest.raises(ValueError):
            demo.beta = bad
    demo.beta = 0.25
    assert demo.beta == 0.25 and M.FusedDemonstrationRollout(mono, K, actor=pol).agent == "own"
    mono.close()
    press.close()
