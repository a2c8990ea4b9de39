"""Training the modular pair in the env it is deployed in.

The reference trains its sorting agent in Env_1 (random press actions) and its pressing agent in Env_2 (a frozen
sorter), then judges the pair in Env_3_Monolith.step(mode='model'), which neither saw.  `ModularTrainer` alternates
one modular collection in Env_3 (`FusedModularRollout`: both agents act side by side, one launch) with one
`PPOLearner.update` per agent on that agent's view of the rollout - each on its own reward component, or both on the
team reward.  An agent without a learner is frozen: it acts by argmax and its weights are never touched.

On a labelled collector (`expert_labels=True`) the rule-based controller teaches in the same loop: a
`PPOLearner(bc_coef=...)` finds its agent's half of the label in its view (`expert_actions`), and an `ImitationLearner`
is updated on `demo_view(who)` - DAgger on the states the pair itself visits, with `learn(beta=...)` mixing the expert
into the stepping.
"""
from __future__ import annotations

from typing import Optional

from .episodes import evaluate_rollout
from .imitation import ImitationLearner
from .learner import PPOLearner, training_loop

AGENTS = ("sort", "press")


class ModularTrainer:
    """collector: a `FusedModularRollout` (or its twin, with reward="team").  sort_learner / press_learner: the
    `PPOLearner` of that agent - or an `ImitationLearner`, which needs a labelled collector -, or None to freeze it; at
    least one, and each over the collector's own agent.  The two may be of different kinds.
    reward: "own" - each PPO learner trains on its agent's component of the step reward - or "team", both on the sum
    (an `ImitationLearner`'s critic always regresses on the team reward's `returns`, when the collector has a `gamma`)."""

    def __init__(self, collector, sort_learner: Optional[PPOLearner] = None, press_learner: Optional[PPOLearner] = None,
                 reward: str = "own"):
        if sort_learner is None and press_learner is None:
            raise ValueError("at least one learner is required")
        if reward not in ("own", "team"):
            raise ValueError(f"reward must be 'own' or 'team', not {reward!r}")
        if sort_learner is not None and sort_learner.policy is not collector.sort_agent:
            raise ValueError("sort_learner must train the collector's sort_agent")
        if press_learner is not None and press_learner.policy is not collector.press_agent:
            raise ValueError("press_learner must train the collector's press_agent")
        self.collector, self.reward = collector, reward
        self.learners = {"sort": sort_learner, "press": press_learner}
        if any(isinstance(l, ImitationLearner) for l in self.learners.values()) and not getattr(collector, "expert_labels", False):
            raise ValueError("an ImitationLearner needs the expert's labels: construct the collector with expert_labels=True")
        self.episode_stats = None  # learn(episode_stats=True): the EpisodeStats whose carry spans the iterations

    def _on_policy_only(self) -> list:
        """The agents whose learner is a PPO learner proper: their rows must be the agents' own."""
        return [who for who in AGENTS
                if self.learners[who] is not None and not isinstance(self.learners[who], ImitationLearner)]

    def learn(self, iterations: int, callback=None, episode_stats: bool = False, eval_env=None, eval_freq: int = 0,
              n_eval_episodes: int = 10, first_iteration: int = 0, beta=None) -> list:
        """Per iteration one `collect()` (a frozen agent deterministic), then one update per learner present: a
        `PPOLearner` on `view(...)` with `progress_remaining = 1 - (it + 1) / iterations`, as `PPOLearner.learn` sets it;
        an `ImitationLearner` on `demo_view(who)`.  Returns one record per
        iteration: {"sort": mean stats, "press": mean stats} for the learners present, "reward" (the team reward per
        env-step), "reward_sort", "reward_press" (its parts; absent when the collector does not fill them).
        beta (a labelled collector's mixture): a number, or a function of the fraction of iterations done (it / iterations,
        from 0 towards 1); it is written into `collector.beta` before each `collect()`, as `ImitationLearner.learn` does,
        and each record then carries `beta` and, under "expert_share", the share of rows the expert stepped.  A
        `PPOLearner` together with a beta > 0 is refused: its rows would not be on-policy.  None: nothing is set, and the
        refusal reads the collector's own beta.
        episode_stats=True: `episodes`, `ep_rew_mean`, `ep_len_mean` over the episodes that ended in that rollout, on
        the team reward.  eval_env (an Env_3 handle of its own) with eval_freq > 0: every eval_freq-th record gains
        `eval_mean_reward` / `eval_std_reward` from `evaluate_rollout(eval_env, "model", ...)` with both agents - the
        reference's "PPO Modular" scenario."""
        col = self.collector
        if beta is not None and not getattr(col, "expert_labels", False):
            raise ValueError("beta needs a collector constructed with expert_labels=True")

        def collect(it):
            # the collector's own beta when none is given here: a collector constructed with beta > 0 is refused alike
            value = getattr(col, "beta", 0.0) if beta is None else float(beta(it / int(iterations)) if callable(beta) else beta)
            if value > 0.0 and self._on_policy_only():
                raise ValueError(f"beta = {value} > 0 with a PPOLearner for {self._on_policy_only()}: the expert would step "
                                 "rows PPO takes for the agents' own (use bc_coef, or an ImitationLearner)")
            if beta is not None:
                col.beta = value
            return col.collect(sort_deterministic=self.learners["sort"] is None,
                               press_deterministic=self.learners["press"] is None)

        def step(data, progress_remaining):
            rec = {"reward": float(data["rewards"].mean())}
            for who in AGENTS:
                if data.get(f"rewards_{who}") is not None:
                    rec[f"reward_{who}"] = float(data[f"rewards_{who}"].mean())
            if beta is not None:
                rec.update(beta=col.beta, expert_share=float(data["expert_stepped"].float().mean()))
            for who in AGENTS:
                learner = self.learners[who]
                if isinstance(learner, ImitationLearner):
                    rec[who] = learner.update(col.demo_view(who))["mean"]
                elif learner is not None:
                    rec[who] = learner.update(col.view(who, self.reward), progress_remaining=progress_remaining)["mean"]
            return rec

        def evaluate():
            return evaluate_rollout(eval_env, "model", n_eval_episodes=n_eval_episodes, sort_agent=col.sort_agent,
                                    press_agent=col.press_agent, press_agent_maskable=col.press_masked)

        return training_loop(iterations, collect, step, first_iteration=first_iteration,
                             stats_owner=self if episode_stats else None, stats_device=col.env.device if episode_stats else None,
                             evaluate=None if eval_env is None else evaluate, eval_freq=eval_freq, callback=callback)
