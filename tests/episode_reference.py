"""numpy restatement of the episode accounting, written from the header comment of csrc/mse_episode_math.h and from
stable-baselines3's evaluate_policy, not from the C code.

    scan()             one call of mse_episode_scan / mse_episode_scan_host on a State (carry, counts, ledger)
    sb3_evaluate()     evaluate_policy's counting loop over recorded step-major rewards and dones
    exact_*()          math.fsum-based sum, mean and population std, and the error bounds DESIGN.md 4.13 derives

A return is np.cumsum over the float64 image of the float32 rewards, restarted after each episode end: cumsum adds
sequentially, which is the header's "one double add per step, in step order"."""
import math

import numpy as np

U = 2.0 ** -53  # unit roundoff of float64


def targets_for(n_eval_episodes, n_envs):
    """episode_count_targets = np.array([(n_eval_episodes + i) // n_envs for i in range(n_envs)])"""
    return np.array([(n_eval_episodes + i) // n_envs for i in range(n_envs)], dtype=np.int32)


def ends_from_starts(episode_starts, last_dones):
    """step k ended an episode iff episode_starts[k + 1] != 0, last_dones at k = K - 1; row 0 is not read"""
    return np.concatenate([episode_starts[1:], last_dones[None, :]], axis=0) != 0


def starts_from_ends(ends, first_row):
    """the collectors' form of the same episode ends: (episode_starts, last_dones); first_row is arbitrary"""
    starts = np.concatenate([first_row[None, :], ends[:-1]], axis=0).astype(np.uint8)
    return starts, ends[-1].astype(np.uint8)


class State:
    def __init__(self, n, slots=0, targets=None):
        self.n, self.slots = n, slots
        self.run_return = np.zeros(n, np.float64)
        self.run_length = np.zeros(n, np.int32)
        self.ep_count = np.zeros(n, np.int32)
        self.targets = None if targets is None else np.asarray(targets, np.int32)
        self.ledger_return = np.full((slots, n), np.nan, np.float64) if slots else None
        self.ledger_length = np.full((slots, n), -1, np.int32) if slots else None
        self.counted = []  # every counted episode (return, length, env), ledger overflow included, in (env, step) order


def scan(state, rewards, ends):
    """rewards f32[K, N], ends bool[K, N].  Returns the counted episodes of this call as (return, length) lists."""
    K, n = rewards.shape
    out_r, out_l = [], []
    for i in range(n):
        r = rewards[:, i].astype(np.float64)
        ret, length, cnt = state.run_return[i], int(state.run_length[i]), int(state.ep_count[i])
        at = 0
        for k in np.flatnonzero(ends[:, i]):
            seg = np.cumsum(np.concatenate([[ret], r[at:k + 1]]))  # ((ret + r0) + r1) + ..
            ep_ret, ep_len = seg[-1], length + (k + 1 - at)
            if state.targets is None or cnt < state.targets[i]:
                if state.slots and cnt < state.slots:
                    state.ledger_return[cnt, i], state.ledger_length[cnt, i] = ep_ret, ep_len
                out_r.append(float(ep_ret))
                out_l.append(ep_len)
                state.counted.append((float(ep_ret), ep_len, i))
                cnt += 1
            ret, length, at = 0.0, 0, k + 1
        if at < K:
            ret = np.cumsum(np.concatenate([[ret], r[at:]]))[-1]
            length += K - at
        state.run_return[i], state.run_length[i], state.ep_count[i] = ret, length, cnt
    return out_r, out_l


def all_returns(rewards_seq, ends_seq):
    """Every episode return of consecutive calls with no targets (all are counted), vectorised over the envs: the
    same sequential float64 adds, one vector add per step."""
    ret = np.zeros(rewards_seq[0].shape[1], np.float64)
    out = []
    for rewards, ends in zip(rewards_seq, ends_seq):
        for k in range(rewards.shape[0]):
            ret = ret + rewards[k].astype(np.float64)
            out.append(ret[ends[k]])
            ret = np.where(ends[k], 0.0, ret)
    return np.concatenate(out)


def sb3_evaluate(rewards, dones, n_eval_episodes):
    """evaluate_policy's loop on recorded steps (rewards f32[T, N], dones [T, N]) from a fresh reset:
        current_rewards += rewards; current_lengths += 1
        for i in range(n_envs):
            if episode_counts[i] < episode_count_targets[i] and dones[i]:
                episode_rewards.append(current_rewards[i]); episode_lengths.append(current_lengths[i])
                episode_counts[i] += 1
            (on done) current_rewards[i] = 0; current_lengths[i] = 0
    until every count has reached its target; the returns are accumulated in float64 from the float32 rewards."""
    T, n = rewards.shape
    targets = targets_for(n_eval_episodes, n)
    counts = np.zeros(n, np.int64)
    cur_r, cur_l = np.zeros(n, np.float64), np.zeros(n, np.int64)
    ep_r, ep_l = [], []
    for t in range(T):
        if (counts >= targets).all():
            break
        cur_r += rewards[t].astype(np.float64)
        cur_l += 1
        for i in range(n):
            if dones[t, i]:
                if counts[i] < targets[i]:
                    ep_r.append(float(cur_r[i]))
                    ep_l.append(int(cur_l[i]))
                    counts[i] += 1
                cur_r[i], cur_l[i] = 0.0, 0
    assert (counts >= targets).all(), "the recording is too short"
    return ep_r, ep_l


# ---- exact values and the derived bounds ----------------------------------------------------------------
def exact_sum(x):
    return math.fsum(x)


def sum_bound(x):
    """any order of count - 1 float64 additions: (count - 1) u sum|x|"""
    return (len(x) - 1) * U * math.fsum(np.abs(np.asarray(x, np.float64)))


def exact_mean_std(x):
    n = len(x)
    mean = math.fsum(x) / n
    return mean, math.sqrt(math.fsum((v - mean) ** 2 for v in x) / n)


def mean_bound(x):
    """(n + 1) u A with A = mean|x|: (n - 1) u A from the sum, u |mean| <= u A from the division, u A for the rounding of
    the fsum-based value it is compared with"""
    n = len(x)
    return (n + 1) * U * math.fsum(abs(v) for v in x) / n


def std_bound(x):
    """u ((n + 1) A + (n + 12) / 2 sigma): a mean off by e moves the population std by at most |e| (sum (x - m)^2 =
    sum (x - mean)^2 + n (m - mean)^2); each (x - m)^2 carries 3 u, the sum of n non-negative terms (n - 1) u, the
    division u, halved by the square root that adds u of its own: (n + 5) / 2 u sigma; the fsum-based value carries
    (3 + 1 + 1) / 2 + 1 = 3.5 u sigma of its own"""
    n = len(x)
    _, sigma = exact_mean_std(x)
    return U * ((n + 1) * math.fsum(abs(v) for v in x) / n + (n + 12) / 2 * sigma)
