"""The reference's policy-quality scenarios that need no trained model, at scale.

utils/benchmark_models.py:126-147 runs `Env_3_Monolith` for STEPS_TEST = 200 steps (main.py:42,50: noise 0) per seed and
sums the reward; utils/benchmark_plot_summary.py:6-17 quotes, over 10 seeds, Random -84.28 +- 22.29 and Rule-Based
44.03 +- 1.10 with masking, Random -109.36 +- 6.29 and Rule-Based 43.20 +- 1.07 without.  Here every seed 1..N is an env
lane: one fused rollout per scenario (rule-based and masked-uniform policies run on the device; the unmasked random
scenario steps with uniform actions over all 22).  Not a parity target (the reference's random mode draws from the
global np.random); the rule-based run is, and tests/test_gpu_api.py checks it seed by seed against the reference.

The scenarios with trained agents (utils/benchmark_models.py:152-172) run Env_3_Monolith.step(mode='model'): PPO Sort-Only
(a sorting agent, the press part drawn from the env's rng_pressing), PPO Modular (sorting + pressing agent, with and
without masking) - both as one fused rollout per 50 steps (BatchedSortingEnv.rollout(policy="model"), mse_rollout_model)
- and PPO Monolith (FusedPolicyRollout, deterministic).  The agents are local `torch.save`d SB3 `policy.state_dict()`
files (--sort-weights / --press-weights / --mono-weights); without one, random-init weights of the same architecture
stand in, and the row says so: its number is not comparable to the paper.  "mode='model', no agents" is the env-stream
random baseline.  --time prints env-steps/s of the fused model rollout against ModelRolloutCollector (one round of
launches per step) for each agent combination at --envs envs and K = --k steps.

    python tools/benchmark_scenarios.py [--envs 65536] [--sort-weights F] [--press-weights F] [--mono-weights F]
    python tools/benchmark_scenarios.py --time [--envs 65536] [--k 200]
    python tools/benchmark_scenarios.py --plant [--envs 4096]      the plant ledger beside the reward (multi-launch stepping)
    python tools/benchmark_scenarios.py --planner 1 4 16 [--envs 10] [--planner-streams fresh] [--planner-samples 1]
                                                                   the lookahead planner (mse_lookahead) at these horizons
    python tools/benchmark_scenarios.py --planner 1 2 4 8 --envs 10 --planner-policy F [--planner-base network] [--planner-leaf]
                                                                   a learned network inside the forks (mse_lookahead_net): its
                                                                   actor as the base policy, its critic as the leaf value
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import marl_sortingenv_amd as M  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=65536)
ap.add_argument("--sort-weights", default=None, help="torch.save'd SB3 policy.state_dict() of the sorting agent (13 -> 2)")
ap.add_argument("--press-weights", default=None, help="... of the pressing agent (16 -> 11)")
ap.add_argument("--mono-weights", default=None, help="... of the monolithic agent (29 -> 22)")
ap.add_argument("--time", action="store_true", help="env-steps/s of the fused model rollout vs ModelRolloutCollector")
ap.add_argument("--k", type=int, default=200, help="steps per rollout for --time")
ap.add_argument("--plant", action="store_true",
                help="also print the plant ledger of the scenarios (evaluate_plant: one episode per seed through the all-env "
                     "trace, 50 x 320 B x envs of device memory): the return's parts, press log, overflow, bales, deviation")
ap.add_argument("--planner", type=int, nargs="+", default=None, metavar="H",
                help="only the planner scenario: at every step each env takes the action BatchedSortingEnv.lookahead(H) ranks "
                     "first (every action tried on a fork, followed by H - 1 rule-based steps), one row per horizon")
ap.add_argument("--planner-streams", default="fresh", choices=("fresh", "own"), help="the forks' streams ('own' is clairvoyant)")
ap.add_argument("--planner-samples", type=int, default=1, help="forks per candidate action")
ap.add_argument("--planner-base", default="rule_based", choices=("rule_based", "random", "network"),
                help="the forks' base policy; 'network': the argmax of the --planner-policy actor (mse_lookahead_net)")
ap.add_argument("--planner-policy", default=None, metavar="FILE",
                help="the network inside the planner's forks (29 -> 22): a state_dict as tools/train_ppo.py --save writes it")
ap.add_argument("--planner-leaf", action="store_true",
                help="add the --planner-policy critic's value of the state a fork stands in after H steps (bootstrapped lookahead)")
args = ap.parse_args()
if (args.planner_leaf or args.planner_base == "network") and not args.planner_policy:
    ap.error("--planner-leaf and --planner-base network need --planner-policy FILE")
n, T = args.envs, 200


def make():
    return M.BatchedSortingEnv(kind="mono", num_envs=n, device=0, base_seed=1, max_steps=T, noise_sorting=0.0,
                               balesize=200, auto_reset=True)  # exactly one episode is stepped


def total_reward(env, policy, masked=True):
    tot = torch.zeros((n,), dtype=torch.float64, device="cuda")
    if policy == "unmasked_random":
        g = torch.Generator(device="cuda").manual_seed(2024)
        for _ in range(T):
            a = torch.randint(0, env.num_actions, (n,), generator=g, device="cuda", dtype=torch.int32)
            _, rew, _, _ = env.step(a, use_action_masking=False, want_reward64=True)
            tot += env.reward64
        return tot
    K = 50
    buf = env.alloc_rollout(K, obs=False, mask=False)
    for _ in range(T // K):
        env.rollout(K, policy_seed=2024, buffers=buf, policy=policy, use_action_masking=masked)
        tot += buf["reward"].double().sum(dim=0)
    return tot




def agent(path, obs_dim, n_actions, seed):
    """(MlpPolicy, label suffix): the state dict at `path`, else random-init weights with a fixed seed."""
    if path:
        return M.MlpPolicy.from_state_dict(torch.load(path, map_location="cpu"), device=0), ""
    return M.MlpPolicy.random_init(obs_dim, n_actions, seed=seed), "  [random-init weights, not comparable to the paper]"


def model_reward(env, sort_agent, press_agent, masked, maskable=True):
    tot = torch.zeros((n,), dtype=torch.float64, device="cuda")
    K = 50
    buf = env.alloc_rollout(K, obs=False, mask=False)
    for _ in range(T // K):
        env.rollout(K, buffers=buf, policy="model", sort_agent=sort_agent, press_agent=press_agent,
                    press_agent_maskable=maskable, use_action_masking=masked)
        tot += buf["reward"].double().sum(dim=0)
    return tot


def mono_reward(env, policy, masked):
    tot = torch.zeros((n,), dtype=torch.float64, device="cuda")
    K = 50
    coll = M.FusedPolicyRollout(env, policy, K)
    for _ in range(T // K):
        tot += coll.collect(deterministic=True, use_action_masking=masked)["rewards"].double().sum(dim=0)
    return tot


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3


if args.planner:
    from marl_sortingenv_amd.plant import evaluate_plant, format_summary

    kw = dict(streams=args.planner_streams, n_samples=args.planner_samples, base_policy=args.planner_base)
    shown = dict(kw)
    if args.planner_policy:
        net = M.MlpPolicy.from_state_dict(torch.load(args.planner_policy, map_location="cpu"), device=0)
        if args.planner_base == "network":
            kw["base_policy"] = net
        if args.planner_leaf:
            kw["leaf_value"] = net
        shown = dict(shown, leaf_value=args.planner_leaf, policy=os.path.basename(args.planner_policy))
    r = total_reward(make(), "rule_based")
    print(f"{'Rule-Based, masking':24s} {n} seeds: cumulative reward {float(r.mean()):8.2f} +- {float(r.std(unbiased=False)):6.2f}")
    for H in args.planner:
        env = make()
        mean, std = M.evaluate_lookahead(env, n, H, **kw)
        print(f"{'Planner H=' + str(H):24s} {n} seeds: cumulative reward {mean:8.2f} +- {std:6.2f}   ({shown})", flush=True)
        if args.plant:
            print(format_summary(evaluate_plant(M.LookaheadCollector(env, 50, H, gamma=1.0, seed=0, **kw), n_eval_episodes=n)))
        env.close()
    sys.exit(0)

if args.time:
    K = args.k
    sort_ag, _ = agent(args.sort_weights, 13, 2, 1)
    press_ag, _ = agent(args.press_weights, 16, 11, 2)
    for label, s_ag, p_ag in (("no agents", None, None), ("sorting agent", sort_ag, None),
                              ("pressing agent (maskable)", None, press_ag), ("both agents (maskable)", sort_ag, press_ag)):
        env = make()
        buf = env.alloc_rollout(K, sort_obs=True, press_obs=True)
        env.rollout(K, buffers=buf, policy="model", sort_agent=s_ag, press_agent=p_ag)  # warm-up
        t_fused = timed(lambda: env.rollout(K, buffers=buf, policy="model", sort_agent=s_ag, press_agent=p_ag))
        coll = M.ModelRolloutCollector(env, sort_agent=s_ag, press_agent=p_ag)
        coll.collect(2, buffers=buf)  # warm-up
        t_multi = timed(lambda: coll.collect(K, buffers=buf))
        print(f"{label:28s} {n} envs, K={K}: fused {n * K / t_fused / 1e9:7.3f} G env-steps/s   "
              f"ModelRolloutCollector {n * K / t_multi / 1e9:7.3f} G env-steps/s   ({t_multi / t_fused:6.1f}x)")
        env.close()
        del buf
    sys.exit(0)

for label, policy, masked, quoted in (
        ("Random, masking", "random", True, "-84.28 +- 22.29"),
        ("Rule-Based, masking", "rule_based", True, "44.03 +- 1.10"),
        ("Random, no masking", "unmasked_random", False, "-109.36 +- 6.29")):
    r = total_reward(make(), policy, masked)
    print(f"{label:24s} {n} seeds: cumulative reward {float(r.mean()):8.2f} +- {float(r.std()):6.2f}   "
          f"(reference, 10 seeds: {quoted})")
print("Rule-Based, no masking   = the masked run: mode='rule_based' executes its action without validation whatever "
      "use_action_masking is (env_monolith.py:166-184, 262-264); the reference quotes 43.20 +- 1.07 for its second sample")

r = model_reward(make(), None, None, True)
print(f"{'mode=model, no agents':24s} {n} seeds: cumulative reward {float(r.mean()):8.2f} +- {float(r.std()):6.2f}   "
      f"(rng_sorting / rng_pressing draws, masking)")
sort_ag, sort_note = agent(args.sort_weights, 13, 2, 1)
press_ag, press_note = agent(args.press_weights, 16, 11, 2)
mono_ag, mono_note = agent(args.mono_weights, 29, 22, 3)
for label, run, note in (
        ("PPO Sort-Only", lambda: model_reward(make(), sort_ag, None, True), sort_note),
        ("PPO Modular, masking", lambda: model_reward(make(), sort_ag, press_ag, True), sort_note or press_note),
        ("PPO Modular, no masking", lambda: model_reward(make(), sort_ag, press_ag, False), sort_note or press_note),
        ("PPO Monolith, masking", lambda: mono_reward(make(), mono_ag, True), mono_note)):
    r = run()
    print(f"{label:24s} {n} seeds: cumulative reward {float(r.mean()):8.2f} +- {float(r.std()):6.2f}{note}")

if args.plant:
    from marl_sortingenv_amd.plant import evaluate_plant, format_summary

    for label, source in (
            ("Random, masking", lambda e: (e, "random")),
            ("Rule-Based, masking", lambda e: (e, "rule_based")),
            ("mode=model, no agents", lambda e: M.ModelRolloutCollector(e)),
            ("PPO Modular, masking" + (sort_note or press_note), lambda e: M.ModelRolloutCollector(e, sort_ag, press_ag))):
        env = make()
        s = evaluate_plant(source(env), n_eval_episodes=n, k_steps=50)
        print(f"{label}: {n} seeds: cumulative reward {s['mean_reward']:8.2f} +- {s['std_reward']:6.2f}")
        print(format_summary(s))
        env.close()
