"""Shared by tests/test_gpu_checkpoint.py and the child process it starts (not a test module): the tiny training run
the checkpoint tests resume, and what is compared afterwards.

Env_3 (or Env_1 / Env_2), 96 envs (one full 64-row tile and a 32-row tail), n_steps = 8, max_steps = 12 (episodes end and
auto-reset inside rollouts; after 2 iterations = 16 steps an env whose episodes ran their full length is 4 steps into
one), noise_sorting = 0.05 (rng_noise is live), n_epochs = 2, batch_size = 256 (768 rows: 3 minibatches per epoch),
4 iterations with a checkpoint after the 2nd.

    python -m tests.checkpoint_checks CASE CHECKPOINT OUT

is the child: it builds CASE's objects afresh (another policy seed, envs stepped a few times), loads CHECKPOINT, runs the
remaining iterations and writes what `final_state` gives, as a checkpoint file, to OUT."""
import ctypes as C
import sys

import numpy as np

N, K, MAX_STEPS, EPOCHS, BS, ITERS, AT = 96, 8, 12, 2, 256, 4, 2
DIMS = {"sort": (13, 2), "press": (16, 11), "mono": (29, 22)}
LR = 1e-3

# name -> (kind, collector, PPOLearner arguments, learn arguments).  A schedule is named here and made in `build`, so
# every learner gets callables of its own.
CASES = {
    "cpu-host": ("mono", "fused", dict(shuffle="cpu", weight_sync="host"), {}),
    "cpu-device": ("mono", "fused", dict(shuffle="cpu", weight_sync="device"), {}),
    "device-host": ("mono", "fused", dict(shuffle="device", weight_sync="host"), {}),
    "device-device": ("mono", "fused", dict(shuffle="device", weight_sync="device"), {}),
    "matrix": ("mono", "fused", dict(arithmetic="matrix"), {}),
    "schedules": ("mono", "fused", dict(learning_rate="linear", clip_range="linear", clip_range_vf=0.2),
                  dict(explained_variance=True)),
    "target_kl": ("mono", "fused", dict(shuffle="device", weight_sync="device", target_kl="TARGET_KL"), {}),
    "episode_stats": ("mono", "fused", {}, dict(episode_stats=True)),
    "eval": ("mono", "fused", dict(weight_sync="device"), dict(eval_freq=1)),
    "sort": ("sort", "fused", {}, {}),
    "press": ("press", "fused", {}, {}),
    "two_launch": ("mono", "two_launch", dict(shuffle="device"), dict(episode_stats=True)),
}


def build(case, fresh=False, target_kl=None, num_envs=N, max_steps=MAX_STEPS, kind=None, learner_kw=None):
    """-> dict(policy, env, collector, learner, sort_policy, learn_kw).  fresh=True is the resumed side: the same
    constructor arguments, but the policy (and Env_2's frozen sorting policy) start from another `random_init` seed and
    the envs are stepped 5 times first, so a load that restores nothing cannot pass."""
    import marl_sortingenv_amd as M

    ckind, collector, lkw, learn_kw = CASES[case]
    kind = ckind if kind is None else kind
    lkw = dict(lkw, **(learner_kw or {}))
    D, A = DIMS[kind]
    pol = M.MlpPolicy.random_init(D, A, seed=77 if fresh else 31)
    env = M.BatchedSortingEnv(kind=kind, num_envs=num_envs, device=0, base_seed=21, max_steps=max_steps, noise_sorting=0.05,
                              balesize=200, auto_reset=True)
    if fresh:
        for _ in range(5):
            env.step(env.sample_actions(policy_seed=3))
    sort_policy = M.MlpPolicy.random_init(13, 2, seed=78 if fresh else 41) if kind == "press" else None
    if collector == "fused":
        col = M.FusedPolicyRollout(env, pol, K, seed=22, sort_policy=sort_policy)
    else:
        col = M.PolicyRolloutCollector(env, pol, K, sort_policy=sort_policy, seed=22)
    if lkw.get("learning_rate") == "linear":
        lkw["learning_rate"] = lambda p: LR * p
    if lkw.get("clip_range") == "linear":
        lkw["clip_range"] = lambda p: 0.2 * p
    if lkw.get("target_kl") == "TARGET_KL":
        lkw["target_kl"] = target_kl
    learner = M.PPOLearner(pol, **dict(dict(learning_rate=LR, n_epochs=EPOCHS, batch_size=BS, seed=5, ent_coef=0.05), **lkw))
    learn_kw = dict(learn_kw)
    if "eval_freq" in learn_kw:
        eval_env = M.BatchedSortingEnv(kind=kind, num_envs=10, device=0, base_seed=10 ** 6, max_steps=max_steps,
                                       noise_sorting=0.05, balesize=200, auto_reset=True)
        learn_kw["eval_collector"] = M.FusedPolicyRollout(eval_env, pol, max_steps, seed=23)
    return dict(policy=pol, env=env, collector=col, learner=learner, sort_policy=sort_policy, learn_kw=learn_kw)


def policies_of(run):
    return None if run["sort_policy"] is None else {"sort_policy": run["sort_policy"]}


def image(pol):
    import torch

    img = np.empty(int(pol.L.mse_policy_image_floats()), dtype=np.float32)
    assert pol.L.mse_policy_read_image(pol._h, C.c_void_p(img.ctypes.data)) == 0
    return torch.from_numpy(img).view(torch.int32)


def final_state(run):
    """What a finished run is compared by, beyond its records and its last checkpoint file: CPU tensors and numbers."""
    import torch

    torch.cuda.synchronize()
    lrn, env = run["learner"], run["env"]
    ints, dbls, rng = env.get_state()
    out = {"weights": lrn.weights.cpu(), "m": lrn.m.cpu(), "v": lrn.v.cpu(), "grad_norm": lrn.grad_norm.cpu(),
           "step": lrn.step, "epochs_done": lrn.epochs_done, "generator": lrn.generator.get_state().clone(),
           "progress_remaining": lrn.progress_remaining, "learning_rate": lrn.learning_rate, "clip_range": lrn.clip_range,
           "clip_range_vf": lrn.clip_range_vf, "best_mean_reward": lrn.best_mean_reward,
           "ints": ints.cpu(), "dbls": dbls.cpu(), "rng": rng.cpu(), "policy_step": env.policy_step,
           "image": image(run["policy"]), "flat_weights": torch.from_numpy(run["policy"].flat_weights().copy())}
    for name in ("weights", "m", "v", "grad_norm"):  # equality below is of bits: -0.0 is not 0.0, NaN equals itself
        out[name] = out[name].view(torch.int32)
    if lrn.best_weights is not None:
        lrn.restore_best()
        out["restored_best_weights"] = lrn.weights.cpu().view(torch.int32)
        out["restored_best_image"] = image(run["policy"])
    if run["sort_policy"] is not None:
        out["sort_policy_image"] = image(run["sort_policy"])
    return out


def resume(case, checkpoint, out_checkpoint, target_kl=None):
    """The resumed side from start to end -> (run, records, final_state)."""
    import marl_sortingenv_amd as M

    import torch

    run = build(case, fresh=True, target_kl=target_kl)
    before = [image(run["policy"]), run["env"].get_state()[2].clone(), run["learner"].weights.clone()]
    ck = M.load_checkpoint(checkpoint, learner=run["learner"], collector=run["collector"], policies=policies_of(run))
    after = [image(run["policy"]), run["env"].get_state()[2], run["learner"].weights]
    assert not any(torch.equal(a, b) for a, b in zip(before, after)), "the fresh objects must start somewhere else"
    assert ck["loaded"] == ["collector"] + (["policies['sort_policy']"] if run["sort_policy"] is not None else []) + ["learner"]
    assert ck["iteration"] == AT and ck["iterations"] == ITERS and len(ck["history"]) == AT
    records = run["learner"].learn(run["collector"], ITERS, first_iteration=ck["iteration"], history=ck["history"],
                                   checkpoint_path=out_checkpoint, checkpoint_freq=AT, **run["learn_kw"])
    return run, records, final_state(run)


def main(argv):
    import marl_sortingenv_amd as M

    case, checkpoint, out = argv[1:4]
    target_kl = float(argv[4]) if len(argv) > 4 else None
    run, records, state = resume(case, checkpoint, out + ".last", target_kl=target_kl)
    M.save_checkpoint(out, iteration=ITERS, iterations=ITERS, history=records, extra=state)


if __name__ == "__main__":
    main(sys.argv)
