"""Times the episode accounting.

    python tools/bench_episodes.py --scan     # mse_episode_scan at [16, 65 536] and [16, 2^20] beside the same accounting in
                                              # torch ops; run it under `rocprofv3 --kernel-trace --stats` for kernel times
    python tools/bench_episodes.py --learn    # one learn() iteration at 65 536 envs with and without episode_stats=True,
                                              # alternating, three timed runs each
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import marl_sortingenv_amd as M  # noqa: E402


def torch_accounting(rewards, starts, last, run_return, run_length, totals):
    """The same accounting in torch ops on the same tensors: a running float64 return per env, closed at each end mark."""
    K = rewards.shape[0]
    for k in range(K):
        run_return += rewards[k].double()
        run_length += 1
        ended = (starts[k + 1] if k + 1 < K else last) != 0
        totals[0] += ended.sum()
        totals[1] += torch.where(ended, run_return, torch.zeros_like(run_return)).sum()
        totals[2] += torch.where(ended, run_length, torch.zeros_like(run_length)).sum()
        run_return.masked_fill_(ended, 0.0)
        run_length.masked_fill_(ended, 0)


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def bench_scan():
    K = 16
    for n in (65536, 2 ** 20):
        g = torch.Generator(device="cuda").manual_seed(n)
        data = {"rewards": torch.randn((K, n), generator=g, device="cuda"),
                "episode_starts": (torch.rand((K, n), generator=g, device="cuda") < 0.02).to(torch.uint8),
                "last_dones": (torch.rand((n,), generator=g, device="cuda") < 0.02).to(torch.uint8)}
        stats = M.EpisodeStats(n, 0)
        t_scan = timed(lambda: stats.update(data), 200)
        rr, rl = torch.zeros(n, dtype=torch.float64, device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda")
        tot = torch.zeros(3, dtype=torch.float64, device="cuda")
        t_torch = timed(lambda: torch_accounting(data["rewards"], data["episode_starts"], data["last_dones"], rr, rl, tot), 20)
        floor_bytes = 5 * K * n + 24 * n  # 5 B/row, and the carry's 8 + 4 B read and written per env
        print(f"[{K}, {n}]: mse_episode_scan (scan + fold, host clock over 200 enqueued calls) {t_scan * 1e6:.1f} us = "
              f"{floor_bytes / t_scan / 1e9:.0f} GB/s of its {floor_bytes} B floor; torch ops {t_torch * 1e6:.1f} us "
              f"({t_torch / t_scan:.1f} x)")


def bench_learn():
    n, K = 65536, 16
    pol = M.MlpPolicy.random_init(29, 22, seed=0)
    env = M.BatchedSortingEnv(kind="mono", num_envs=n, device=0, base_seed=0, max_steps=50, auto_reset=True)
    col = M.FusedPolicyRollout(env, pol, K, seed=0)
    learner = M.PPOLearner(pol, ent_coef=0.05, shuffle="device")
    times = {False: [], True: []}
    for rep in range(4):
        for flag in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            learner.learn(col, 1, episode_stats=flag)
            torch.cuda.synchronize()
            if rep > 0:
                times[flag].append(time.perf_counter() - t0)
    for flag, ts in times.items():
        print(f"learn() iteration, {n} envs x {K} steps, episode_stats={flag}: " + " / ".join(f"{t * 1e3:.2f}" for t in ts) + " ms")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--scan", action="store_true")
    ap.add_argument("--learn", action="store_true")
    args = ap.parse_args()
    if args.scan:
        bench_scan()
    if args.learn:
        bench_learn()
