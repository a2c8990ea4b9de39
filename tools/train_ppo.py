"""Train one of the three envs with the on-device PPO learner, from MlpPolicy.random_init.

    python tools/train_ppo.py --kind mono --envs 4096 --steps 16 --iterations 20
    python tools/train_ppo.py --kind mono --shuffle device   # the epoch permutations from mse_ppo_shuffle, not the CPU
    python tools/train_ppo.py --kind mono --episode-stats --eval-every 5   # ep_rew_mean / ep_len_mean of the training rollouts and
                                                          # evaluate_policy on 10 envs of their own every 5th iteration
    python tools/train_ppo.py --kind mono --time          # rows/s of mse_ppo_loss_grad beside torch f32 autograd, and one
                                                          # update() with shuffle="cpu" and shuffle="device"; then the weight
                                                          # hand-over alone and inside update(), host against device
    python tools/train_ppo.py --kind mono --weight-sync device --target-kl 0.03   # repack on the device; SB3's early stop
    python tools/train_ppo.py --kind mono --arithmetic matrix   # the gradient's products on the f32 matrix cores
    python tools/train_ppo.py --kind mono --time --time-section arithmetic   # only the last block of --time: loss_grad
                                                          # (with and without value clipping) and update() with
                                                          # arithmetic="fma" against "matrix"
    python tools/train_ppo.py --kind mono --clip-range-vf 0.2 --lr-schedule linear --clip-schedule linear --explained-variance
                                                          # SB3's clip_range_vf, linear decay of the learning rate and the
                                                          # clip range, train/explained_variance per iteration
    python tools/train_ppo.py --kind mono --iterations 20 --checkpoint run_{iteration}.pt --checkpoint-every 5
                                                          # one file after every 5th iteration: learner, envs, history
    python tools/train_ppo.py --kind mono --iterations 20 --resume run_10.pt   # the same command line plus --resume:
                                                          # iterations 10 .. 19 of the same run, bit for bit
    python tools/train_ppo.py --kind modular --reward own --eval-every 10   # the sorting (13 -> 2) and the pressing agent
                                                          # (16 -> 11) side by side in Env_3, each on its own reward
                                                          # component (--reward team: both on the sum); the evaluation
                                                          # is the reference's "PPO Modular" scenario
    python tools/train_ppo.py --kind mono --pretrain rule_based --pretrain-iterations 20 --eval-every 10
                                                          # clone the env's rule-based controller first (ImitationLearner on
                                                          # a DemonstrationCollector), then PPO from the cloned weights;
                                                          # --kind modular clones both agents from their own views
    python tools/train_ppo.py --time --time-section bc    # mse_bc_loss_grad beside mse_ppo_loss_grad, both arithmetics
    python tools/train_ppo.py --kind mono --pretrain rule_based --dagger --beta-schedule linear --eval-every 10
                                                          # DAgger: the clone (or a beta-mixture of clone and expert)
                                                          # acts, the expert labels every visited state, in one launch
                                                          # per collection (FusedDemonstrationRollout); --beta-schedule
                                                          # one | linear | first: beta 1 throughout (pure cloning), 1 - the
                                                          # fraction of iterations done, or 1 in the first iteration only
    python tools/train_ppo.py --kind mono --pretrain rule_based --dagger --bc-coef 1 --bc-schedule linear --eval-every 10
                                                          # PPO with an imitation term: the rule-based controller labels
                                                          # the rollout PPO trains on (expert_labels=True) and the loss
                                                          # gains bc_coef * bc_loss; linear: bc_coef times
                                                          # progress_remaining, which reaches 0 in the last iteration
    python tools/train_ppo.py --time --time-section demo  # collect() of FusedDemonstrationRollout beside
                                                          # DemonstrationCollector(actor=student) and the plain policy rollout
    python tools/train_ppo.py --kind modular --pretrain rule_based --dagger --beta-schedule linear --eval-every 10
                                                          # the pair cloned jointly on the states it visits itself: a
                                                          # labelled FusedModularRollout (one launch: both agents, the
                                                          # expert's label in its two halves, the beta-mixture) and one
                                                          # ImitationLearner per agent; then PPO
    python tools/train_ppo.py --kind modular --pretrain rule_based --bc-coef 1 --bc-schedule linear --eval-every 10
                                                          # the pair's PPO with each agent's half of the label in its loss
    python tools/train_ppo.py --time --time-section modular_demo  # the labelled modular launch beside the plain one and the twin;
                                                          # any --kind, and only when named: --time alone (section
                                                          # 'all') does not run it
    python tools/train_ppo.py --kind mono --view preview --pretrain rule_based --dagger --eval-every 10
                                                          # the mono policy on the in-step view: it is shown the observation
                                                          # after the step's flow update, as the modular agents are
                                                          # (mse_rollout_policy_preview: cloning, DAgger, --bc-coef and the
                                                          # evaluation all on that view)
    python tools/train_ppo.py --kind mono --pretrain lookahead --horizon 8 --eval-every 10
                                                          # the teacher is the lookahead planner (LookaheadCollector: every
                                                          # action tried on a fork of the env and followed by H - 1 rule-based
                                                          # steps, one mse_lookahead launch per step); --dagger: the clone steps
    python tools/train_ppo.py --kind mono --pretrain lookahead --horizon 8 --dagger --planner-self --eval-every 10
                                                          # expert iteration: the policy being cloned is the planner's base
                                                          # policy and leaf value (mse_lookahead_net, the current weights)
    python tools/train_ppo.py --time --time-section preview  # the preview launch (plain, with labels, with the mixture) beside
                                                          # the plain policy kernel at 65 536 and 262 144 envs; only when named
    python -m torch.distributed.run --nproc-per-node 8 tools/train_ppo.py --kind mono --envs 262144 --data-parallel
                                                          # one process per GPU: every rank steps its block of the global
                                                          # envs and trains on its own rows; per minibatch the ranks
                                                          # all-reduce four doubles and the gradient sums (RCCL); rank 0 prints
    python tools/train_ppo.py --time --time-section exchange  # update() with a one-rank exchange, collectives forced on, beside
                                                          # the plain update(): the fixed overhead of the phase split

Prints the mean reward per env-step and the learner's mean statistics per iteration (a record that learning happens).
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import marl_sortingenv_amd as M  # noqa: E402
from marl_sortingenv_amd.policy import _shapes  # noqa: E402

KINDS = {"sort": "Env_1_Sorting", "press": "Env_2_Pressing", "mono": "Env_3_Monolith"}


def torch_loss(w, D, A, obs, mask, actions, old_logp, adv, ret, clip, ent_coef, vf_coef):
    """MaskablePPO.train's loss for one minibatch in torch ops on the tensors' device (f32)."""
    import torch.nn.functional as F

    parts, at = [], 0
    for s in _shapes(D, A):
        n = 1
        for v in s:
            n *= v
        parts.append(w[at:at + n].reshape(s))
        at += n
    w1, b1, w2, b2, wa, ba, v1, c1, v2, c2, wv, bv = parts
    adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    hp = torch.tanh(F.linear(torch.tanh(F.linear(obs, w1, b1)), w2, b2))
    hv = torch.tanh(F.linear(torch.tanh(F.linear(obs, v1, c1)), v2, c2))
    logits = torch.where(mask, F.linear(hp, wa, ba), torch.tensor(-1e8, device=obs.device))
    logsm = torch.log_softmax(logits, dim=1)
    logp = logsm.gather(1, actions.long().unsqueeze(1)).squeeze(1)
    ratio = torch.exp(logp - old_logp)
    pl = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - clip, 1 + clip)).mean()
    vl = F.mse_loss(ret, F.linear(hv, wv, bv).squeeze(1))
    el = torch.where(mask, logsm * logsm.exp(), torch.zeros((), device=obs.device)).sum(dim=1).mean()
    return pl + ent_coef * el + vf_coef * vl


def time_loss_grad(args):
    D, A = M.OBS_DIM[args.kind], M.NUM_ACTIONS[args.kind]
    pol = M.MlpPolicy.random_init(D, A, seed=args.seed)
    for n in (256, 4096, 65536):
        K = 16
        env = M.BatchedSortingEnv(kind=args.kind, num_envs=n, device=0, base_seed=args.seed, max_steps=50, auto_reset=True)
        col = M.FusedPolicyRollout(env, pol, K, seed=args.seed)
        learner = M.PPOLearner(pol, ent_coef=0.05)
        data = M.compute_gae(col.collect())
        rows = K * n
        stats = torch.zeros(8, device="cuda")

        def fused():
            learner.loss_grad(data, None, rows, stats)

        flat = [data[k].reshape(rows, -1) if data[k].dim() == 3 else data[k].reshape(rows)
                for k in ("observations", "action_masks", "actions", "log_probs", "advantages", "returns")]
        flat[1] = flat[1].bool()
        w = learner.weights.clone().requires_grad_(True)

        def autograd():
            w.grad = None
            torch_loss(w, D, A, *flat, 0.2, 0.05, 0.5).backward()

        res = {}
        for name, fn in (("mse_ppo_loss_grad", fused), ("torch f32 autograd", autograd)):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            reps = 20 if rows <= 65536 else 5
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            res[name] = (time.perf_counter() - t0) / reps
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            M.compute_gae(data)
        torch.cuda.synchronize()
        t_gae = (time.perf_counter() - t0) / 20
        print(f"{args.kind} rows={rows}: mse_gae {t_gae * 1e6:.1f} us = {17 * rows / t_gae / 1e9:.0f} GB/s of its 17 B/row")
        # one update() beside the collect() that feeds it, in both shuffle modes: one warm-up each, then three timed
        # updates each, alternating
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        col.collect()
        torch.cuda.synchronize()
        t_col = time.perf_counter() - t0
        learners = {mode: M.PPOLearner(pol, ent_coef=0.05, shuffle=mode) for mode in ("cpu", "device")}
        t_upd = {mode: [] for mode in learners}
        for rep in range(4):
            for mode, lrn in learners.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                lrn.update(data)
                torch.cuda.synchronize()
                if rep > 0:
                    t_upd[mode].append(time.perf_counter() - t0)
        print(f"{args.kind} rows={rows}: " + ", ".join(f"{k} {v * 1e6:.1f} us ({rows / v / 1e6:.1f} M rows/s)" for k, v in res.items())
              + f"; collect {t_col * 1e6:.0f} us, update (10 epochs x 4 minibatches) "
              + ", ".join(f"shuffle={mode} " + " / ".join(f"{t * 1e3:.2f}" for t in ts) + " ms" for mode, ts in t_upd.items()))


def time_exchange(args):
    """The fixed overhead of the phase split: update() with a GradientExchange at world size 1, the collectives forced on
    over RCCL (three phases and two all-reduces per minibatch), beside the plain update() (one mse_ppo_loss_grad per
    minibatch) on the same rollout, at time_loss_grad's sizes.  One warm-up each, then three timed updates each,
    alternating; every timed region ends in a device synchronise.  What the two collectives cost between GPUs is not in it."""
    import torch.distributed as dist

    from marl_sortingenv_amd.sharding import GradientExchange

    D, A = M.OBS_DIM[args.kind], M.NUM_ACTIONS[args.kind]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    own_group = not dist.is_initialized()
    if own_group:
        dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29547", rank=0, world_size=1, device_id=dev)
    try:
        ex = GradientExchange(device=dev, force_collective=True)
        for n in (256, 4096, 65536):
            K = 16
            pol = M.MlpPolicy.random_init(D, A, seed=args.seed)
            env = M.BatchedSortingEnv(kind=args.kind, num_envs=n, device=0, base_seed=args.seed, max_steps=50, auto_reset=True)
            data = M.FusedPolicyRollout(env, pol, K, seed=args.seed).collect()
            kw = dict(ent_coef=0.05, shuffle="device", weight_sync="device", arithmetic=args.arithmetic)
            learners = {"plain": M.PPOLearner(pol, **kw), "exchange": M.PPOLearner(pol, exchange=ex, **kw)}
            times = {name: [] for name in learners}
            for rep in range(4):
                for name, lrn in learners.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    lrn.update(data)
                    torch.cuda.synchronize()
                    if rep > 0:
                        times[name].append(time.perf_counter() - t0)
            print(f"{args.kind} rows={K * n}: update (10 epochs x 4 minibatches, shuffle=device, weight_sync=device, "
                  f"arithmetic={args.arithmetic}) " + ", ".join(f"{name} " + " / ".join(f"{t * 1e3:.2f}" for t in ts) + " ms"
                                                              for name, ts in times.items()))
    finally:
        if own_group:
            dist.destroy_process_group()


def time_weight_sync(args):
    """The weight hand-over, host against device, at 4 096, 65 536 and 2^20 rows: `load_weights` against
    `load_weights_device(sync=True)` alone, and one update() with shuffle="device" under each `weight_sync`.  One warm-up
    each, then three timed calls each, alternating; every timed region ends in a device synchronise."""
    D, A = M.OBS_DIM[args.kind], M.NUM_ACTIONS[args.kind]
    K = 16

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for rows in (4096, 65536, 2 ** 20):
        n = rows // K
        pol = M.MlpPolicy.random_init(D, A, seed=args.seed)
        env = M.BatchedSortingEnv(kind=args.kind, num_envs=n, device=0, base_seed=args.seed, max_steps=50, auto_reset=True)
        col = M.FusedPolicyRollout(env, pol, K, seed=args.seed)
        data = col.collect()
        w = torch.from_numpy(pol.flat_weights()).cuda()
        loads = {"load_weights": lambda: pol.load_weights(w), "load_weights_device": lambda: pol.load_weights_device(w, sync=True)}
        learners = {mode: M.PPOLearner(pol, ent_coef=0.05, shuffle="device", weight_sync=mode) for mode in ("host", "device")}
        updates = {f"update weight_sync={mode}": (lambda lrn=lrn: lrn.update(data)) for mode, lrn in learners.items()}
        for group in (loads, updates):
            times = {name: [] for name in group}
            for rep in range(4):
                for name, fn in group.items():
                    t = timed(fn)
                    if rep > 0:
                        times[name].append(t)
            unit = 1e6 if group is loads else 1e3
            print(f"{args.kind} rows={rows}: " + ", ".join(
                f"{name} " + " / ".join(f"{t * unit:.1f}" if group is loads else f"{t * unit:.2f}" for t in ts)
                + (" us" if group is loads else " ms") for name, ts in times.items()))


def time_arithmetic(args):
    """arithmetic="fma" against "matrix" at 4 096, 65 536 and 2^20 rows: `loss_grad` alone (rows_dev = NULL, back-to-back
    calls ending in one synchronise, the time per call) and one update() (10 epochs x 4 minibatches, shuffle="device",
    weight_sync="device").  One process, the two forms alternating, one warm-up each, then three timed repetitions each."""
    D, A = M.OBS_DIM[args.kind], M.NUM_ACTIONS[args.kind]
    K = 16
    forms = ("fma", "matrix")
    for rows in (4096, 65536, 2 ** 20):
        n = rows // K
        pol = M.MlpPolicy.random_init(D, A, seed=args.seed)
        env = M.BatchedSortingEnv(kind=args.kind, num_envs=n, device=0, base_seed=args.seed, max_steps=50, auto_reset=True)
        col = M.FusedPolicyRollout(env, pol, K, seed=args.seed)
        data = M.compute_gae(col.collect())
        stats = torch.zeros(8, device="cuda")
        calls = 20 if rows <= 65536 else 5
        learners = {f: M.PPOLearner(pol, ent_coef=0.05, arithmetic=f) for f in forms}
        # the same call with value clipping (the VCLIP instantiation of each kernel, through mse_ppo_loss_grad_vclip)
        learners.update({f + "+vclip": M.PPOLearner(pol, ent_coef=0.05, arithmetic=f, clip_range_vf=0.2) for f in forms})
        updaters = {f: M.PPOLearner(pol, ent_coef=0.05, shuffle="device", weight_sync="device", arithmetic=f) for f in forms}

        def loss_grads(lrn):
            for _ in range(calls):
                lrn.loss_grad(data, None, rows, stats)

        for what, group, per in (("loss_grad", {f: (lambda lrn=lrn: loss_grads(lrn)) for f, lrn in learners.items()}, calls),
                                 ("update", {f: (lambda lrn=lrn: lrn.update(data)) for f, lrn in updaters.items()}, 1)):
            times = {f: [] for f in group}
            for r in range(4):
                for f, fn in group.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    if r > 0:
                        times[f].append((time.perf_counter() - t0) / per)
            unit, name = (1e6, "us") if what == "loss_grad" else (1e3, "ms")
            worst = min(times["fma"]) / max(times["matrix"])
            best = max(times["fma"]) / min(times["matrix"])
            print(f"{args.kind} rows={rows}: {what} " + ", ".join(
                f"arithmetic={f} " + " / ".join(f"{t * unit:.1f}" if unit == 1e6 else f"{t * unit:.2f}" for t in ts) + f" {name}"
                for f, ts in times.items()) + f"; fma / matrix {worst:.2f} .. {best:.2f}")


def time_bc(args):
    """`mse_bc_loss_grad` and `mse_ppo_bc_loss_grad` beside `mse_ppo_loss_grad` on Env_3's shape at 4 096, 65 536 and 2^20
    rows, both arithmetics: rows_dev = NULL, one warm-up, then back-to-back calls ending in one synchronise, the time per
    call; the six calls alternating, three timed repetitions each.  The cloning call gets the PPO rollout's rows with the
    rule's labels; the PPO call with the imitation term gets the PPO rollout with the labels of a twin's states beside it
    (any labels cost the same)."""
    D, A = M.OBS_DIM["mono"], M.NUM_ACTIONS["mono"]
    K = 16
    for rows in (4096, 65536, 2 ** 20):
        n = rows // K
        pol = M.MlpPolicy.random_init(D, A, seed=args.seed)
        env = M.BatchedSortingEnv(kind="mono", num_envs=n, device=0, base_seed=args.seed, max_steps=50, auto_reset=True)
        data = M.compute_gae(M.FusedPolicyRollout(env, pol, K, seed=args.seed).collect())
        demo_env = M.BatchedSortingEnv(kind="mono", num_envs=n, device=0, base_seed=args.seed, max_steps=50, auto_reset=True)
        demo = M.DemonstrationCollector(demo_env, K).collect()
        stats = torch.zeros(12, device="cuda")
        calls = 20 if rows <= 65536 else 5
        labelled = dict(data, expert_actions=demo["actions"])
        group = {}
        for f in ("fma", "matrix"):
            group[f"ppo {f}"] = (M.PPOLearner(pol, ent_coef=0.05, arithmetic=f), data)
            group[f"bc {f}"] = (M.ImitationLearner(pol, ent_coef=0.05, arithmetic=f), demo)
            group[f"ppo+bc {f}"] = (M.PPOLearner(pol, ent_coef=0.05, arithmetic=f, bc_coef=1.0), labelled)
        times = {name: [] for name in group}
        for r in range(4):
            for name, (lrn, d) in group.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(calls):
                    lrn.loss_grad(d, None, rows, stats)
                torch.cuda.synchronize()
                if r > 0:
                    times[name].append((time.perf_counter() - t0) / calls)
        print(f"mono rows={rows}: loss_grad " + ", ".join(f"{name} " + " / ".join(f"{t * 1e6:.1f}" for t in ts) + " us"
                                                           for name, ts in times.items()))


def time_demo(args):
    """`collect()` of `FusedDemonstrationRollout` (beta 0, 0.5 and, without an actor, 1) beside its multi-launch twin
    `DemonstrationCollector(actor=student)` and `FusedPolicyRollout` forced to the plain kernel (rollout_pipeline = 2: the
    same loop without the label and the selection), Env_3, at 4 096 envs x 50 steps and 65 536 x 16: HIP events around
    each call, one warm-up, then three timed calls each, the collectors alternating."""
    D, A = M.OBS_DIM["mono"], M.NUM_ACTIONS["mono"]
    pol = M.MlpPolicy.random_init(D, A, seed=args.seed, precision="f16x3")

    def env(n, **kw):
        return M.BatchedSortingEnv(kind="mono", num_envs=n, device=0, base_seed=args.seed, max_steps=50, auto_reset=True, **kw)

    for n, K in ((4096, 50), (65536, 16)):
        group = {
            "fused beta=0": M.FusedDemonstrationRollout(env(n), K, actor=pol, beta=0.0, seed=args.seed),
            "fused beta=0.5": M.FusedDemonstrationRollout(env(n), K, actor=pol, beta=0.5, seed=args.seed),
            "fused expert only": M.FusedDemonstrationRollout(env(n), K),
            "twin actor=student": M.DemonstrationCollector(env(n), K, actor=pol, seed=args.seed),
            "twin expert only": M.DemonstrationCollector(env(n), K),
            "policy rollout (plain kernel)": M.FusedPolicyRollout(env(n, rollout_pipeline=2), pol, K, seed=args.seed),
            "labelled rollout": M.FusedPolicyRollout(env(n), pol, K, seed=args.seed, expert_labels=True),
            "labelled twin": M.PolicyRolloutCollector(env(n), pol, K, seed=args.seed, expert_labels=True),
        }
        times = {name: [] for name in group}
        for r in range(4):
            for name, col in group.items():
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                col.collect()
                stop.record()
                stop.synchronize()
                if r > 0:
                    times[name].append(start.elapsed_time(stop))
        print(f"mono {n} envs x {K} steps: collect() " + ", ".join(
            f"{name} " + " / ".join(f"{t:.3f}" for t in ts) + f" ms ({n * K / min(ts) / 1e3:.1f} M steps/s)" for name, ts in times.items()))


def time_modular_demo(args):
    """`collect()` of the labelled `FusedModularRollout` (beta 0 and 0.5) beside the plain one and the multi-launch twin
    `ModularRolloutCollector(expert_labels=True)`, Env_3, K = 16, noise 0, at 65 536 and 262 144 envs: HIP events around each
    call, one warm-up, then three timed calls each, the collectors alternating (the modular rollout's procedure)."""
    sort_ag = M.MlpPolicy.random_init(13, 2, seed=args.seed, precision="f16x3")
    press_ag = M.MlpPolicy.random_init(16, 11, seed=args.seed + 1, precision="f16x3")

    def env(n):
        return M.BatchedSortingEnv(kind="mono", num_envs=n, device=0, base_seed=args.seed, max_steps=50, auto_reset=True)

    K = 16
    for n in (65536, 262144):
        group = {
            "plain": M.FusedModularRollout(env(n), sort_ag, press_ag, K),
            "labelled beta=0": M.FusedModularRollout(env(n), sort_ag, press_ag, K, expert_labels=True, beta=0.0),
            "labelled beta=0.5": M.FusedModularRollout(env(n), sort_ag, press_ag, K, expert_labels=True, beta=0.5),
            "labelled twin beta=0.5": M.ModularRolloutCollector(env(n), sort_ag, press_ag, K, expert_labels=True, beta=0.5),
        }
        times = {name: [] for name in group}
        for r in range(4):
            for name, col in group.items():
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                col.collect()
                stop.record()
                stop.synchronize()
                if r > 0:
                    times[name].append(start.elapsed_time(stop))
        print(f"modular {n} envs x {K} steps: collect() " + ", ".join(
            f"{name} " + " / ".join(f"{t:.3f}" for t in ts) + f" ms ({n * K / min(ts) / 1e3:.1f} M steps/s)" for name, ts in times.items()))


def time_preview(args):
    """`collect()` of `FusedPolicyRollout(view="preview")` (threshold 0, no labels) beside `FusedPolicyRollout` held to the plain
    kernel (rollout_pipeline = 2: the same loop without the flow update on a copy and the second observation build), then the
    preview launch with labels and with the beta = 0.5 mixture, Env_3, K = 16, f16x3, noise 0, at 65 536 and 262 144 envs: HIP
    events around each call, one warm-up, then five timed calls each, the collectors alternating."""
    pol = M.MlpPolicy.random_init(29, 22, seed=args.seed, precision="f16x3")

    def env(n, **kw):
        return M.BatchedSortingEnv(kind="mono", num_envs=n, device=0, base_seed=args.seed, max_steps=50, auto_reset=True, **kw)

    K = 16
    for n in (65536, 262144):
        group = {
            "plain policy kernel": M.FusedPolicyRollout(env(n, rollout_pipeline=2), pol, K, seed=args.seed),
            "preview": M.FusedPolicyRollout(env(n), pol, K, seed=args.seed, view="preview"),
            "preview + labels": M.FusedPolicyRollout(env(n), pol, K, seed=args.seed, view="preview", expert_labels=True),
            "preview demo beta=0.5": M.FusedDemonstrationRollout(env(n), K, actor=pol, beta=0.5, seed=args.seed, agent="preview"),
        }
        times = {name: [] for name in group}
        for r in range(6):
            for name, col in group.items():
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                col.collect()
                stop.record()
                stop.synchronize()
                if r > 0:
                    times[name].append(start.elapsed_time(stop))
        base = min(times["plain policy kernel"])
        print(f"mono {n} envs x {K} steps: collect() " + ", ".join(
            f"{name} " + " / ".join(f"{t:.3f}" for t in ts) + f" ms ({n * K / min(ts) / 1e3:.1f} M steps/s, x{min(ts) / base:.3f})"
            for name, ts in times.items()))


BETA_SCHEDULES = {"one": 1.0, "linear": lambda f: 1.0 - f, "first": lambda f: 1.0 if f == 0.0 else 0.0}


def pretrain(args, pol, env_kind, agent, name, eval_col=None):
    """--pretrain rule_based: clone the env's rule-based controller into `pol` before PPO (DemonstrationCollector on envs
    of its own, ImitationLearner); the PPO learner constructed afterwards starts from the cloned weights."""
    env = M.BatchedSortingEnv(kind=env_kind, num_envs=args.envs, device=0, base_seed=args.seed + 2 * 10 ** 6,
                              max_steps=args.max_steps, auto_reset=True)
    planner = args.pretrain == "lookahead"
    if planner:  # the planner labels the env's own observation; with --dagger the student steps, without it the planner
        # --planner-self: expert iteration - the student is the base policy and the leaf value of the planner that labels
        # it (mse_lookahead_net reads the handle's weights at every launch, so each collect() plans with the last update's)
        self_kw = dict(base_policy=pol, leaf_value=pol) if args.planner_self else {}
        col = M.LookaheadCollector(env, args.steps, args.horizon, actor=pol if args.dagger else None, seed=args.seed + 7,
                                   n_samples=args.lookahead_samples, **self_kw)
    elif args.dagger:
        col = M.FusedDemonstrationRollout(env, args.steps, actor=pol, beta=1.0, seed=args.seed + 7, mix_seed=args.seed + 8,
                                          agent="preview" if agent == "preview" else "own")
    else:
        col = M.DemonstrationCollector(env, args.steps, agent=agent)
    il = M.ImitationLearner(pol, learning_rate=args.pretrain_lr, n_epochs=args.pretrain_epochs, batch_size=args.batch_size,
                            seed=args.seed, shuffle=args.shuffle, weight_sync=args.weight_sync, arithmetic=args.arithmetic)
    print(f"cloning {f'the lookahead planner (H = {args.horizon})' if planner else 'the rule-based controller'} into {name} ({pol.obs_dim} -> {pol.n_actions}): {args.pretrain_iterations} "
          f"iterations of {args.envs} envs x {args.steps} steps, {args.pretrain_epochs} epochs each, lr {args.pretrain_lr:g}"
          + (", the student is the planner's base policy and leaf value" if planner and args.planner_self else "")
          + (", the student steps" if planner and args.dagger else
             f", DAgger with beta schedule '{args.beta_schedule}'" if args.dagger else ""))

    def show(it, rec):
        print(f"bc {it:3d} reward/step of the {'mixture' if args.dagger else 'expert'} {rec['reward']:+.4f} loss {rec['loss']:+.4f} "
              f"bc {rec['bc_loss']:.4f} vf {rec['value_loss']:.4f} accuracy {rec['accuracy']:.4f} unusable {rec['unusable']:.4f}"
              + (f" beta {rec['beta']:.3f} expert share {rec['expert_share']:.4f}" if "beta" in rec else "")
              + (f" eval {rec['eval_mean_reward']:+.3f} +- {rec['eval_std_reward']:.3f}" if "eval_mean_reward" in rec else ""))

    return il.learn(col, args.pretrain_iterations, callback=show, eval_collector=eval_col,
                    eval_freq=args.eval_every if eval_col is not None else 0,
                    beta=BETA_SCHEDULES[args.beta_schedule] if args.dagger and not planner else None)


def pretrain_modular_dagger(args, sort_ag, press_ag):
    """--kind modular --pretrain rule_based --dagger: both agents cloned in ONE loop on the states the pair itself visits - a
    labelled FusedModularRollout on envs of its own (one launch per collection: both agents act, the rule-based controller labels
    every state in its two halves, and a beta-mixture of pair and expert steps), one ImitationLearner per agent on its
    demo_view."""
    env = M.BatchedSortingEnv(kind="mono", num_envs=args.envs, device=0, base_seed=args.seed + 2 * 10 ** 6,
                              max_steps=args.max_steps, auto_reset=True)
    col = M.FusedModularRollout(env, sort_ag, press_ag, args.steps, sort_seed=args.seed + 7, press_seed=args.seed + 8,
                                expert_labels=True, beta=1.0, mix_seed=args.seed + 9, gamma=0.99)
    ils = [M.ImitationLearner(pol, learning_rate=args.pretrain_lr, n_epochs=args.pretrain_epochs, batch_size=args.batch_size,
                              seed=args.seed + i, shuffle=args.shuffle, weight_sync=args.weight_sync, arithmetic=args.arithmetic)
           for i, pol in enumerate((sort_ag, press_ag))]
    print(f"cloning the rule-based controller into both agents, jointly: {args.pretrain_iterations} iterations of {args.envs} envs x "
          f"{args.steps} steps, {args.pretrain_epochs} epochs each, lr {args.pretrain_lr:g}, DAgger with beta schedule "
          f"'{args.beta_schedule}'")

    def show(it, rec):
        print(f"bc {it:3d} reward/step of the mixture {rec['reward']:+.4f} beta {rec['beta']:.3f} expert share {rec['expert_share']:.4f}")
        for who in ("sort", "press"):
            r = rec[who]
            print(f"       {who:5s} loss {r['loss']:+.4f} bc {r['bc_loss']:.4f} vf {r['value_loss']:.4f} accuracy {r['accuracy']:.4f} "
                  f"unusable {r['unusable']:.4f}")

    return M.ModularTrainer(col, ils[0], ils[1]).learn(args.pretrain_iterations, callback=show,
                                                       beta=BETA_SCHEDULES[args.beta_schedule])


def train_modular(args):
    """--kind modular: both agents in Env_3_Monolith, one FusedModularRollout and one PPOLearner each (ModularTrainer).
    --bc-coef: the rollout is labelled and each learner's loss keeps its agent's half of the rule-based label."""
    if args.time or args.resume or args.checkpoint:
        raise SystemExit("--kind modular takes neither --time nor --checkpoint / --resume")
    if args.dagger and not args.pretrain:
        raise SystemExit("--dagger goes with --pretrain rule_based")
    sort_ag = M.MlpPolicy.random_init(13, 2, seed=args.seed, precision="f16x3")
    press_ag = M.MlpPolicy.random_init(16, 11, seed=args.seed + 1, precision="f16x3")
    if args.pretrain and args.dagger:
        pretrain_modular_dagger(args, sort_ag, press_ag)
    elif args.pretrain:
        pretrain(args, sort_ag, "mono", "sort", "the sorting agent")
        pretrain(args, press_ag, "mono", "press", "the pressing agent")
    env = M.BatchedSortingEnv(kind="mono", num_envs=args.envs, device=0, base_seed=args.seed, max_steps=args.max_steps,
                              auto_reset=True)
    col = M.FusedModularRollout(env, sort_ag, press_ag, args.steps, sort_seed=args.seed, press_seed=args.seed + 1,
                                expert_labels=args.bc_coef is not None)
    lr = (lambda p: args.lr * p) if args.lr_schedule == "linear" else args.lr
    clip = (lambda p: 0.2 * p) if args.clip_schedule == "linear" else 0.2
    bc_coef = (lambda p: args.bc_coef * p) if args.bc_coef is not None and args.bc_schedule == "linear" else args.bc_coef
    learners = [M.PPOLearner(pol, learning_rate=lr, n_epochs=args.epochs, batch_size=args.batch_size, ent_coef=args.ent_coef,
                             seed=args.seed + i, shuffle=args.shuffle, weight_sync=args.weight_sync, target_kl=args.target_kl,
                             arithmetic=args.arithmetic, clip_range=clip, clip_range_vf=args.clip_range_vf, bc_coef=bc_coef)
                for i, pol in enumerate((sort_ag, press_ag))]
    print(f"Env_3_Monolith, sorting agent (13 -> 2) + pressing agent (16 -> 11), reward={args.reward}, {args.envs} envs x "
          f"{args.steps} steps per iteration" + (f", bc_coef {args.bc_coef:g} {args.bc_schedule}" if args.bc_coef is not None else ""))

    def show(it, rec):
        print(f"it {it:3d} reward/step {rec['reward']:+.4f} = sort {rec['reward_sort']:+.4f} + press {rec['reward_press']:+.4f}")
        for who in ("sort", "press"):
            r = rec[who]
            print(f"       {who:5s} loss {r['loss']:+.4f} pg {r['policy_loss']:+.4f} vf {r['value_loss']:.4f} "
                  f"ent {-r['entropy_loss']:.3f} kl {r['approx_kl']:.4f} clip {r['clip_fraction']:.3f}"
                  + (f" bc_loss {r['bc_loss']:.4f} bc_accuracy {r['bc_accuracy']:.4f}" if "bc_loss" in r else ""))
        if "episodes" in rec:
            print(f"       episodes {rec['episodes']:6d} ep_rew_mean {rec['ep_rew_mean']:+.3f} ep_len_mean {rec['ep_len_mean']:.1f}")
        if "eval_mean_reward" in rec:
            print(f"       eval (mode='model', both agents) {rec['eval_mean_reward']:+.3f} +- {rec['eval_std_reward']:.3f}")

    eval_env = None
    if args.eval_every > 0:
        eval_env = M.BatchedSortingEnv(kind="mono", num_envs=10, device=0, base_seed=args.seed + 10 ** 6, max_steps=args.max_steps,
                                       auto_reset=True)
        if args.pretrain:
            mean, std = M.evaluate_rollout(eval_env, "model", sort_agent=sort_ag, press_agent=press_ag, press_agent_maskable=col.press_masked)
            print(f"cloned pair, before PPO: eval (mode='model', both agents) {mean:+.3f} +- {std:.3f}")
    M.ModularTrainer(col, learners[0], learners[1], reward=args.reward).learn(
        args.iterations, callback=show, episode_stats=args.episode_stats, eval_env=eval_env, eval_freq=args.eval_every)
    if args.eval_plant:  # why the pair scores what it scores: the plant ledger of 10 episodes in mode='model'
        from marl_sortingenv_amd.plant import evaluate_plant, format_summary

        plant_env = M.BatchedSortingEnv(kind="mono", num_envs=10, device=0, base_seed=args.seed + 10 ** 6, max_steps=args.max_steps,
                                        auto_reset=True)
        s = evaluate_plant(M.ModelRolloutCollector(plant_env, sort_ag, press_ag, press_agent_maskable=col.press_masked),
                           k_steps=min(args.max_steps, 50))
        print(f"plant ledger (mode='model', both agents): eval {s['mean_reward']:+.3f} +- {s['std_reward']:.3f}")
        print(format_summary(s))
    if args.save:
        torch.save({"sort_agent": sort_ag.state_dict(), "press_agent": press_ag.state_dict()}, args.save)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", choices=sorted(KINDS) + ["modular"], default="mono")
    ap.add_argument("--view", choices=("own", "preview"), default="own",
                    help="--kind mono: what the policy is shown - the observation the previous step returned, or (preview) the one "
                         "after the step's flow update, as Env_3_Monolith.step shows a stored mono_agent")
    ap.add_argument("--reward", choices=("own", "team"), default="own",
                    help="--kind modular: each agent trains on its own component of the step reward, or both on the sum")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--batch-size", type=int, default=None)
    ap.add_argument("--lr", type=float, default=3e-4)
    ap.add_argument("--ent-coef", type=float, default=0.05)
    ap.add_argument("--max-steps", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--shuffle", choices=("cpu", "device"), default="cpu",
                    help="where an epoch's row permutation comes from: the seeded CPU generator or mse_ppo_shuffle")
    ap.add_argument("--weight-sync", choices=("host", "device"), default="host",
                    help="how an update hands its weights to the policy: through the host repack, or one repack launch on the device")
    ap.add_argument("--target-kl", type=float, default=None,
                    help="SB3's target_kl: stop an update after the minibatch whose approx_kl exceeds 1.5 times this")
    ap.add_argument("--episode-stats", action="store_true",
                    help="print the episodes that ended in each rollout with their mean return and length (SB3's ep_rew_mean)")
    ap.add_argument("--eval-plant", action="store_true",
                    help="after training print the plant ledger of 10 evaluation episodes (evaluate_plant): the return's sort "
                         "and press parts, press log counts, overflow rate, bales per material, average bale deviation")
    ap.add_argument("--eval-every", type=int, default=0,
                    help="every this many iterations evaluate_policy (10 deterministic episodes) and keep the best weights")
    ap.add_argument("--arithmetic", choices=("fma", "matrix"), default="fma",
                    help="how the gradient's products are formed: fmaf chains on the vector unit, or the f32 matrix cores")
    ap.add_argument("--clip-range-vf", type=float, default=None,
                    help="SB3's clip_range_vf: clip the value prediction to this distance from the rollout's (default: off)")
    ap.add_argument("--lr-schedule", choices=("constant", "linear"), default="constant",
                    help="linear: --lr times progress_remaining, which reaches 0 in the last iteration")
    ap.add_argument("--clip-schedule", choices=("constant", "linear"), default="constant",
                    help="linear: the clip range 0.2 times progress_remaining")
    ap.add_argument("--explained-variance", action="store_true",
                    help="print SB3's train/explained_variance of each rollout's values against its returns")
    ap.add_argument("--pretrain", choices=("rule_based", "lookahead"), default=None,
                    help="clone the env's rule-based controller into the policy first (ImitationLearner), then run PPO from there; "
                         "--kind modular clones the sorting and the pressing agent from their own views of Env_3.  lookahead: the "
                         "teacher is the planner instead (LookaheadCollector: every action tried on a fork and followed by "
                         "--horizon - 1 rule-based steps); with --dagger the policy being cloned steps the envs")
    ap.add_argument("--horizon", type=int, default=8, metavar="H", help="with --pretrain lookahead: the planner's horizon")
    ap.add_argument("--lookahead-samples", type=int, default=1, metavar="M", help="with --pretrain lookahead: forks per candidate")
    ap.add_argument("--planner-self", action="store_true",
                    help="with --pretrain lookahead: expert iteration - the policy being cloned is the planner's base policy (argmax) "
                         "and its critic the leaf value (mse_lookahead_net), so every collection plans with the current weights")
    ap.add_argument("--pretrain-iterations", type=int, default=20, metavar="N",
                    help="with --pretrain: collections of --envs x --steps demonstrations, each followed by one update")
    ap.add_argument("--pretrain-epochs", type=int, default=4, help="with --pretrain: epochs per update")
    ap.add_argument("--pretrain-lr", type=float, default=1e-3, help="with --pretrain: the cloning learning rate")
    ap.add_argument("--dagger", action="store_true",
                    help="with --pretrain: the policy being cloned (or a beta-mixture of it and the expert) steps the envs and the "
                         "expert labels every visited state, one launch per collection (FusedDemonstrationRollout)")
    ap.add_argument("--beta-schedule", choices=sorted(BETA_SCHEDULES), default="linear",
                    help="with --dagger: the share of steps the expert takes - 'one': all of them (pure cloning), 'linear': 1 minus "
                         "the fraction of cloning iterations done, 'first': all in the first iteration, none afterwards")
    ap.add_argument("--bc-coef", type=float, default=None, metavar="X",
                    help="PPO with an imitation term: the loss gains X times the cross-entropy of the rule-based controller's "
                         "action at every rollout row (the collector then labels its rollout: expert_labels=True)")
    ap.add_argument("--bc-schedule", choices=("const", "linear"), default="const",
                    help="with --bc-coef: linear is X times progress_remaining, which reaches 0 in the last iteration")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--time-section", choices=("all", "loss_grad", "weight_sync", "arithmetic", "bc", "demo", "modular_demo", "preview",
                                               "exchange"),
                    default="all",
                    help="with --time: run one block of the timings only; 'all' is every block but modular_demo (four collectors "
                         "at 262 144 envs, the multi-launch twin among them), preview and exchange (it brings up a process "
                         "group), which run only when named, with any --kind")
    ap.add_argument("--data-parallel", action="store_true",
                    help="run under `python -m torch.distributed.run --nproc-per-node R`: every rank steps its block of the "
                         "--envs global envs on its own GPU and keeps its rows; the update exchanges moments and gradient sums "
                         "(PPOLearner(exchange=GradientExchange())); rank 0 prints.  --batch-size counts rows per rank")
    ap.add_argument("--checkpoint", default=None, metavar="PATH",
                    help="write the whole run state here (save_checkpoint); an {iteration} field keeps one file per checkpoint")
    ap.add_argument("--checkpoint-every", type=int, default=0, metavar="N",
                    help="with --checkpoint: after every N-th iteration (default: once, after the last)")
    ap.add_argument("--resume", default=None, metavar="PATH",
                    help="continue the run of a --checkpoint file at its iteration; the other arguments must be the ones it was "
                         "started with (a differing hyperparameter or env is refused by name)")
    ap.add_argument("--save", default=None, help="torch.save the trained state_dict (SB3 names) here")
    args = ap.parse_args()
    if args.view == "preview" and args.kind != "mono":
        raise SystemExit("--view preview is the mono policy's in-step view: it goes with --kind mono")
    if args.pretrain == "lookahead" and (args.kind == "modular" or args.view != "own"):
        raise SystemExit("--pretrain lookahead labels the env's own observation: it goes with --kind sort | press | mono and --view own")
    if args.pretrain == "lookahead" and args.horizon < 1:
        raise SystemExit("--horizon must be >= 1")
    if args.planner_self and args.pretrain != "lookahead":
        raise SystemExit("--planner-self goes with --pretrain lookahead")
    if args.kind == "modular" and not (args.time and args.time_section in ("modular_demo", "preview")):
        return train_modular(args)
    if args.time:
        for name, fn in (("loss_grad", time_loss_grad), ("weight_sync", time_weight_sync), ("arithmetic", time_arithmetic),
                         ("bc", time_bc), ("demo", time_demo)):
            if args.time_section in ("all", name):
                fn(args)
        if args.time_section == "modular_demo":  # only by name: four collectors at 262 144 envs, the multi-launch twin among them
            time_modular_demo(args)
        if args.time_section == "preview":
            time_preview(args)
        if args.time_section == "exchange":
            time_exchange(args)
        return
    D, A = M.OBS_DIM[args.kind], M.NUM_ACTIONS[args.kind]
    pol = M.MlpPolicy.random_init(D, A, seed=args.seed)
    exchange, rank, device = None, 0, 0
    if args.data_parallel:
        import torch.distributed as dist

        from marl_sortingenv_amd.sharding import GradientExchange, shard_range

        for flag, name in ((args.bc_coef is not None, "--bc-coef"), (args.explained_variance, "--explained-variance"),
                           (args.pretrain, "--pretrain"), (args.resume or args.checkpoint, "--checkpoint / --resume")):
            if flag:
                raise SystemExit(f"--data-parallel does not go with {name}")
        if "RANK" not in os.environ:
            raise SystemExit("--data-parallel runs under `python -m torch.distributed.run --nproc-per-node R tools/train_ppo.py ...`")
        device = int(os.environ.get("LOCAL_RANK", 0)) % torch.cuda.device_count()
        torch.cuda.set_device(device)
        dist.init_process_group("nccl", device_id=torch.device("cuda", device))  # RCCL: one GPU per rank
        rank, world = dist.get_rank(), dist.get_world_size()
        exchange = GradientExchange(device=torch.device("cuda", device))
        # this rank's contiguous block of the global env indices (ShardedSortingEnv's rule): env g is seeded with seed + g
        # and its policy stream keyed by g, so the rollouts of all ranks together are those of one handle of --envs envs
        start, n_local = shard_range(args.envs, world, rank)
        pol = M.MlpPolicy.random_init(D, A, seed=args.seed, device=device) if device != 0 else pol
        env = M.BatchedSortingEnv(kind=args.kind, num_envs=n_local, device=device, base_seed=args.seed, max_steps=args.max_steps,
                                  auto_reset=True, index_offset=start)
        if rank == 0:
            print(f"data-parallel: {world} ranks, {args.envs} global envs, rank 0 steps envs [{start}, {start + n_local})")
    else:
        env = M.BatchedSortingEnv(kind=args.kind, num_envs=args.envs, device=0, base_seed=args.seed, max_steps=args.max_steps,
                                  auto_reset=True)
    # --bc-coef: the rollout PPO trains on, with the rule's label of every state it visits, in one launch
    col = M.FusedPolicyRollout(env, pol, args.steps, seed=args.seed, expert_labels=args.bc_coef is not None, view=args.view)
    lr = (lambda p: args.lr * p) if args.lr_schedule == "linear" else args.lr
    clip = (lambda p: 0.2 * p) if args.clip_schedule == "linear" else 0.2
    bc_coef = (lambda p: args.bc_coef * p) if args.bc_coef is not None and args.bc_schedule == "linear" else args.bc_coef
    eval_col = None
    if args.eval_every > 0:
        eval_env = M.BatchedSortingEnv(kind=args.kind, num_envs=10, device=device, base_seed=args.seed + 10 ** 6, max_steps=args.max_steps,
                                       auto_reset=True)
        eval_col = M.FusedPolicyRollout(eval_env, pol, min(args.max_steps, 50), seed=args.seed + 1, view=args.view)
    if args.pretrain and not args.resume:  # a resumed run's weights come from its checkpoint
        pretrain(args, pol, args.kind, args.view, "the policy", eval_col if args.dagger else None)
    learner = M.PPOLearner(pol, learning_rate=lr, n_epochs=args.epochs, batch_size=args.batch_size, ent_coef=args.ent_coef,
                           seed=args.seed, shuffle=args.shuffle, weight_sync=args.weight_sync, target_kl=args.target_kl,
                           arithmetic=args.arithmetic, clip_range=clip, clip_range_vf=args.clip_range_vf, bc_coef=bc_coef,
                           exchange=exchange)
    if rank == 0:
        print(f"{KINDS[args.kind]} ({D} -> {A}{', view=preview' if args.view == 'preview' else ''}), {args.envs} envs x {args.steps} steps per iteration, shuffle={args.shuffle}, "
              f"weight_sync={args.weight_sync}, target_kl={args.target_kl}, arithmetic={args.arithmetic}, "
              f"clip_range_vf={args.clip_range_vf}, lr {args.lr_schedule}, clip range {args.clip_schedule}"
              + (f", bc_coef {args.bc_coef:g} {args.bc_schedule}" if args.bc_coef is not None else ""))

    def show(it, rec):
        if rank != 0:  # the statistics are the global ones, identical on every rank; the reward is this rank's envs'
            return
        print(f"it {it:3d} reward/step {rec['reward']:+.4f} loss {rec['loss']:+.4f} pg {rec['policy_loss']:+.4f} "
              f"vf {rec['value_loss']:.4f} ent {-rec['entropy_loss']:.3f} kl {rec['approx_kl']:.4f} clip {rec['clip_fraction']:.3f}")

        if "bc_coef" in rec:
            print(f"       bc_coef {rec['bc_coef']:.4f} bc_loss {rec['bc_loss']:.4f} bc_accuracy {rec['bc_accuracy']:.4f} "
                  f"bc_unusable {rec['bc_unusable']:.4f}")
        if "learning_rate" in rec:
            print(f"       learning_rate {rec['learning_rate']:.3e} clip_range {rec['clip_range']:.4f}")
        if "explained_variance" in rec:
            print(f"       explained_variance {rec['explained_variance']:+.4f}")
        if "in_sync" in rec:
            print(f"       weights identical on all ranks: {rec['in_sync']}")
        if "stopped" in rec:
            print(f"       minibatches run {rec['minibatches_run']}" + (" (stopped on target_kl)" if rec["stopped"] else ""))
        if "episodes" in rec:
            print(f"       episodes {rec['episodes']:6d} ep_rew_mean {rec['ep_rew_mean']:+.3f} ep_len_mean {rec['ep_len_mean']:.1f}")
        if "eval_mean_reward" in rec:
            print(f"       eval {rec['eval_mean_reward']:+.3f} +- {rec['eval_std_reward']:.3f} (best {learner.best_mean_reward:+.3f})")

    if eval_col is not None and args.pretrain and not args.resume:
        mean, std = M.evaluate_policy(eval_col)
        print(f"cloned policy, before PPO: eval {mean:+.3f} +- {std:.3f}")
    first, history = 0, None
    if args.resume:
        ck = M.load_checkpoint(args.resume, learner=learner, collector=col)
        first, history = ck["iteration"], ck["history"]
        if ck["iterations"] is not None and ck["iterations"] != args.iterations:
            print(f"note: the checkpoint was written by a run of {ck['iterations']} iterations, this one has {args.iterations}: "
                  f"progress_remaining, and with it any schedule, continues on the new scale")
        print(f"resuming {args.resume} at iteration {first}; already done:")
        for it, rec in enumerate(history):
            show(it, rec)
        print("continuing:")
    every = args.checkpoint_every if args.checkpoint_every > 0 else args.iterations
    learner.learn(col, args.iterations, callback=show, episode_stats=args.episode_stats, eval_collector=eval_col,
                  eval_freq=args.eval_every, explained_variance=args.explained_variance, first_iteration=first, history=history,
                  checkpoint_path=args.checkpoint, checkpoint_freq=every if args.checkpoint else 0, check_sync=args.data_parallel)
    if eval_col is not None:
        learner.restore_best()
    if args.eval_plant and rank == 0:  # why the policy scores what it scores: the plant ledger of 10 deterministic episodes
        from marl_sortingenv_amd.plant import evaluate_plant, format_summary

        plant_env = M.BatchedSortingEnv(kind=args.kind, num_envs=10, device=device, base_seed=args.seed + 10 ** 6,
                                        max_steps=args.max_steps, auto_reset=True)
        plant_col = M.PolicyRolloutCollector(plant_env, pol, min(args.max_steps, 50), seed=args.seed + 1, view=args.view)
        s = evaluate_plant(plant_col, collect_kwargs={"deterministic": True})
        print(f"plant ledger: eval {s['mean_reward']:+.3f} +- {s['std_reward']:.3f}")
        print(format_summary(s))
    if args.save and rank == 0:
        torch.save(pol.state_dict(), args.save)
    if args.data_parallel:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
