"""CPU: the one training loop (`learner.training_loop`) through its three callers - `PPOLearner.learn`,
`ImitationLearner.learn`, `ModularTrainer.learn` - on plain Python fakes: the exact key order of a record, the order
append -> checkpoint -> callback, the first_iteration / history semantics, the progress_remaining sequence and the
eval_freq cadence.  No device, no library call."""
from types import SimpleNamespace

import pytest
import torch

from marl_sortingenv_amd import learner, modular
from marl_sortingenv_amd.imitation import BC_STAT_NAMES, ImitationLearner
from marl_sortingenv_amd.learner import STAT_NAMES, PPOLearner
from marl_sortingenv_amd.modular import ModularTrainer

EPISODE_KEYS = ["episodes", "ep_rew_mean", "ep_len_mean"]
EVAL_KEYS = ["eval_mean_reward", "eval_std_reward"]
N_ENVS = 6


class Column:
    """What the loop asks of a buffer tensor: a shape and a mean."""

    def __init__(self, mean, shape=(4, N_ENVS)):
        self.value, self.shape = mean, shape

    def mean(self):
        return self.value

    def float(self):
        return self


class FakeStats:
    """Stands for EpisodeStats: logs its calls into the shared event list."""

    events = None

    def __init__(self, num_envs, device):
        self.num_envs, self.device = num_envs, device

    def reset_totals(self):
        self.events.append("stats.reset_totals")

    def update(self, data):
        self.events.append("stats.update")

    def totals(self):
        self.events.append("stats.totals")
        return {"episodes": 3, "mean_return": 1.5, "mean_length": 7.0}


@pytest.fixture
def events(monkeypatch):
    log = []
    monkeypatch.setattr(FakeStats, "events", log)
    monkeypatch.setattr(learner, "EpisodeStats", FakeStats)
    return log


def fake_collector(events, policy=None, **extra):
    def collect(**kw):
        events.append(("collect", kw) if kw else "collect")
        return dict({"rewards": Column(0.25)}, **extra)

    return SimpleNamespace(collect=collect, policy=policy)


def fake_ppo(events, progress, gated=True, scheduled=True, vclip=True):
    ppo = object.__new__(PPOLearner)
    ppo.policy, ppo.device, ppo.episode_stats = object(), "learner-dev", None
    ppo.schedules = {"learning_rate": None} if scheduled else {}
    ppo.learning_rate, ppo.clip_range, ppo.clip_range_vf = 3e-4, 0.2, (0.3 if vclip else None)
    ppo.best_mean_reward, ppo.best_weights, ppo.weights = float("-inf"), None, torch.arange(3.0)

    def update(data, explained_variance=False):
        events.append("update")
        progress.append(ppo.progress_remaining)
        out = {"mean": {name: 0.0 for name in STAT_NAMES}}
        if gated:
            out.update(stopped=False, minibatches_run=4)
        if explained_variance:
            out["explained_variance"] = 0.5
        return out

    ppo.update = update
    return ppo


def test_ppo_learn_records_order_and_cadence(events, monkeypatch):
    progress, saved, called = [], [], []
    ppo = fake_ppo(events, progress)
    means = iter([1.0, 0.5])

    def evaluate_policy(collector, n_eval_episodes):
        events.append("evaluate")
        assert n_eval_episodes == 5
        return next(means), 0.1

    def save_checkpoint(path, learner, collector, policies, iteration, iterations, history):
        events.append("checkpoint")
        # the record is in the history, its callback has not run yet
        assert len(history) == iteration and len(called) == iteration - 1
        saved.append((path, iteration, iterations, policies, learner is ppo))

    monkeypatch.setattr(learner, "evaluate_policy", evaluate_policy)
    monkeypatch.setattr(learner, "save_checkpoint", save_checkpoint)
    col = fake_collector(events)

    def callback(it, rec):
        events.append("callback")
        called.append(it)

    hist = ppo.learn(col, 4, callback=callback, episode_stats=True, eval_collector=fake_collector(events, ppo.policy), eval_freq=2,
                     n_eval_episodes=5, explained_variance=True, checkpoint_path="run_{iteration}.pt", checkpoint_freq=3)
    base = [*STAT_NAMES, "reward", "stopped", "minibatches_run", "learning_rate", "clip_range", "clip_range_vf",
            "explained_variance", *EPISODE_KEYS]
    assert [list(r) for r in hist] == [base, base + EVAL_KEYS, base, base + EVAL_KEYS]
    assert progress == [1.0 - (it + 1) / 4 for it in range(4)] and progress[-1] == 0.0 and ppo.progress_remaining == 0.0
    assert called == [0, 1, 2, 3]
    assert saved == [("run_3.pt", 3, 4, None, True)]
    plain = ["collect", "stats.reset_totals", "stats.update", "update", "stats.totals"]
    assert events == plain + ["callback"] + plain + ["evaluate", "callback"] + plain + ["checkpoint", "callback"] \
        + plain + ["evaluate", "callback"]
    assert isinstance(ppo.episode_stats, FakeStats) and (ppo.episode_stats.num_envs, ppo.episode_stats.device) == (N_ENVS, "learner-dev")
    assert ppo.best_mean_reward == 1.0 and torch.equal(ppo.best_weights, ppo.weights) and ppo.best_weights is not ppo.weights
    assert hist[1]["eval_mean_reward"] == 1.0 and hist[3]["eval_mean_reward"] == 0.5 and hist[3]["eval_std_reward"] == 0.1
    assert (hist[0]["episodes"], hist[0]["ep_rew_mean"], hist[0]["ep_len_mean"]) == (3, 1.5, 7.0)


def test_ppo_learn_defaults_give_the_plain_record(events):
    progress = []
    ppo = fake_ppo(events, progress, gated=False, scheduled=False, vclip=False)
    stats = ppo.episode_stats = FakeStats(N_ENVS, "kept")
    hist = ppo.learn(fake_collector(events), 2, eval_collector=fake_collector(events, ppo.policy))  # eval_freq = 0: never
    assert [list(r) for r in hist] == [[*STAT_NAMES, "reward"]] * 2 and events == ["collect", "update"] * 2
    ppo.learn(fake_collector(events), 1, episode_stats=True)
    assert ppo.episode_stats is stats  # the carry of an EpisodeStats of the right width spans calls
    with pytest.raises(ValueError, match="eval_collector must run this learner's policy"):
        ppo.learn(fake_collector(events), 2, eval_collector=fake_collector(events, object()), eval_freq=1)


def test_first_iteration_and_history(events, monkeypatch):
    progress = []
    ppo = fake_ppo(events, progress, gated=False, scheduled=False, vclip=False)
    col = fake_collector(events)
    before = [{"reward": -1.0}, {"reward": -2.0}]
    hist = ppo.learn(col, 4, first_iteration=2, history=before)
    assert hist[:2] == before and hist is not before and len(before) == 2 and len(hist) == 4
    assert progress == [1.0 - 3 / 4, 0.0]
    assert len(ppo.learn(col, 4, first_iteration=2)) == 2  # no history given: the records of this call alone
    del events[:]
    assert ppo.learn(col, 4, first_iteration=4, history=before) == before and events == []
    for bad in (-1, 5):
        with pytest.raises(ValueError, match=r"first_iteration must be in \[0, iterations = 4\], not " + str(bad)):
            ppo.learn(col, 4, first_iteration=bad)
    for kw in ({"checkpoint_freq": 1}, {"checkpoint_freq": -1, "checkpoint_path": "x.pt"}):
        with pytest.raises(ValueError, match="checkpoint_freq must be >= 0, and > 0 needs a checkpoint_path"):
            ppo.learn(col, 4, **kw)
    assert events == []
    # a collector with a frozen sort_policy: the checkpoint carries it
    saved = []
    monkeypatch.setattr(learner, "save_checkpoint", lambda path, **kw: saved.append((path, kw["policies"], kw["iteration"])))
    col.sort_policy = "frozen"
    ppo.learn(col, 2, checkpoint_path="last.pt", checkpoint_freq=1)
    assert saved == [("last.pt", {"sort_policy": "frozen"}, 1), ("last.pt", {"sort_policy": "frozen"}, 2)]


def test_imitation_learn_records_beta_and_cadence(events, monkeypatch):
    il = object.__new__(ImitationLearner)
    il.policy = object()
    betas = []

    def update(data):  # no progress_remaining: cloning has no schedule
        events.append("update")
        return {"mean": {name: 0.0 for name in BC_STAT_NAMES}}

    il.update = update
    monkeypatch.setattr(learner, "evaluate_policy", lambda collector, n_eval_episodes: (events.append("evaluate"), 2.0, 0.0)[1:])
    col = fake_collector(events, expert_stepped=Column(0.75))
    col.beta = None
    inner = col.collect
    col.collect = lambda: (betas.append(col.beta), inner())[1]  # beta is written before the collection
    called = []
    hist = il.learn(col, 4, callback=lambda it, rec: called.append((it, len(rec))), eval_collector=fake_collector(events, il.policy),
                    eval_freq=3, beta=lambda f: 1.0 - f)
    base = [*dict.fromkeys(BC_STAT_NAMES), "reward", "beta", "expert_share"]
    assert [list(r) for r in hist] == [base, base, base + EVAL_KEYS, base]
    assert betas == [1.0, 0.75, 0.5, 0.25] and [r["beta"] for r in hist] == betas and hist[0]["expert_share"] == 0.75
    assert called == [(0, len(base)), (1, len(base)), (2, len(base) + 2), (3, len(base))]
    assert events == ["collect", "update"] * 2 + ["collect", "update", "evaluate"] + ["collect", "update"]
    assert il.learn(col, 2, beta=0.5)[1]["beta"] == 0.5 and betas[-2:] == [0.5, 0.5]
    col.beta = "untouched"
    plain = il.learn(col, 2)
    assert [list(r) for r in plain] == [[*dict.fromkeys(BC_STAT_NAMES), "reward"]] * 2 and col.beta == "untouched"
    assert il.learn(col, 0) == [] and il.learn(col, -1) == []  # range(iterations) from 0, nothing refused
    with pytest.raises(ValueError, match="eval_collector must run this learner's policy"):
        il.learn(col, 2, eval_collector=fake_collector(events, object()), eval_freq=1)


def test_modular_learn_records_order_and_cadence(events, monkeypatch):
    progress = []
    sort_agent, press_agent = object(), object()

    def update(view, progress_remaining):
        events.append(f"update {view}")
        progress.append(progress_remaining)
        return {"mean": {"loss": 0.0}}

    col = fake_collector(events, rewards_sort=Column(0.1), rewards_press=Column(0.15))
    col.sort_agent, col.press_agent, col.press_masked, col.env = sort_agent, press_agent, True, SimpleNamespace(device="env-dev")
    col.view = lambda who, reward: f"{who}/{reward}"

    def evaluate_rollout(env, policy, n_eval_episodes, sort_agent, press_agent, press_agent_maskable):
        events.append("evaluate")
        assert (env, policy, n_eval_episodes, press_agent_maskable) == ("eval-env", "model", 10, True)
        return 4.0, 0.5

    monkeypatch.setattr(modular, "evaluate_rollout", evaluate_rollout)
    trainer = ModularTrainer(col, sort_learner=SimpleNamespace(policy=sort_agent, update=update), reward="team")
    called = []
    hist = trainer.learn(5, callback=lambda it, rec: called.append(it), episode_stats=True, eval_env="eval-env", eval_freq=2,
                         first_iteration=1)
    base = ["reward", "reward_sort", "reward_press", "sort", *EPISODE_KEYS]
    assert [list(r) for r in hist] == [base + EVAL_KEYS, base, base + EVAL_KEYS, base]  # iterations 1 .. 4: (it + 1) % 2 == 0 at 1, 3
    assert progress == [1.0 - (it + 1) / 5 for it in range(1, 5)] and called == [1, 2, 3, 4]
    frozen_press = ("collect", {"sort_deterministic": False, "press_deterministic": True})  # the agent without a learner
    plain = [frozen_press, "stats.reset_totals", "stats.update", "update sort/team", "stats.totals"]
    assert events == plain + ["evaluate"] + plain + plain + ["evaluate"] + plain
    assert (trainer.episode_stats.num_envs, trainer.episode_stats.device) == (N_ENVS, "env-dev")
    assert hist[0]["sort"] == {"loss": 0.0} and (hist[0]["reward"], hist[0]["reward_sort"], hist[0]["reward_press"]) == (0.25, 0.1, 0.15)
    # both learners, no parts in the rollout (the multi-launch twin), defaults
    col2 = fake_collector(events)
    col2.sort_agent, col2.press_agent = sort_agent, press_agent
    col2.view = col.view
    both = ModularTrainer(col2, SimpleNamespace(policy=sort_agent, update=update), SimpleNamespace(policy=press_agent, update=update))
    del events[:]
    assert [list(r) for r in both.learn(1, eval_env="eval-env")] == [["reward", "sort", "press"]]
    assert events == [("collect", {"sort_deterministic": False, "press_deterministic": False}), "update sort/own", "update press/own"]
