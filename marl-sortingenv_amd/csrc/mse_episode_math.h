// mse_episode_math.h -- episode accounting over rollout buffers (mse_episode.hip), in plain C++ that compiles for the
// host and for the device alike (as mse_ppo_math.h does): k_episode_scan and mse_episode_scan_host run episode_walk,
// k_episode_summary and mse_episode_summary_host run summary_finish, so tests/test_episode_cpu.py can hold the
// arithmetic against tests/episode_reference.py without a GPU.
//
// What it restates: the reference measures a policy in cumulative reward per episode - SB3's Monitor around the
// training env (ep_rew_mean / ep_len_mean), evaluate_policy(model, env, n_eval_episodes) and EvalCallback
// (src/training.py:69,149-157,196-209), np.mean / np.std over per-seed cumulative rewards
// (utils/benchmark_models.py:39), cumulative_reward (src/testing.py:54).
//
// episode_walk, env column i of step-major [K, N] arrays (row stride n), for k = 0 .. K - 1 in that order:
//   1. run_return += (double)rewards[k, i]      one double add per step, in step order, nothing else ever added
//   2. run_length += 1
//   3. the step ended an episode iff
//        dones form:           dones[k, i] != 0
//        episode_starts form:  episode_starts[k + 1, i] != 0 for k < K - 1, last_dones[i] != 0 for k = K - 1
//                              (row 0 of episode_starts is never read)
//   4. an ended episode is COUNTED iff  targets == NULL  or  ep_count[i] < targets[i]   (evaluate_policy's per-env rule:
//      `if episode_counts[i] < episode_count_targets[i]`).  A counted episode
//        - is stored at ledger_return / ledger_length[ep_count[i], i] if a ledger is given and ep_count[i] < slots
//          (slot-major [slots, N]: the lanes of a wave store neighbouring cells),
//        - is added to the lane's Totals (count += 1, sum_return += run_return, sum_length += run_length, min, max),
//        - increments ep_count[i].
//   5. counted or not, run_return = 0 and run_length = 0 after an ended episode.
// run_return / run_length / ep_count are read before step 0 and written back after step K - 1, so a return spans any
// number of calls.  No other cell is written: ledger cells of episodes that did not happen keep what they held.
// A return is therefore the float64 sum, sequential in step order, of the FLOAT32 rewards the buffer holds:
// np.cumsum(r.astype(np.float64)) restarts give the same bits.
//
// The loads of a step do not depend on the carry, so the walk takes kEpisodeChunk steps' rewards and end marks into
// registers first and then runs the dependent double adds over them.
//
// Summary (np.mean / np.std, ddof 0, over the counted ledger entries x_1 .. x_n with lengths l_j):
//   pass 1: n, S = sum x, L = sum l, min, max;  mean = S / n;  mean_length = L / n
//   pass 2: Q = sum (x - mean)^2 with the rounded mean;  std = sqrt(Q / n)
// n = 0 gives NaN for everything but the count.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MSE_EP_HD __host__ __device__ __forceinline__
#else
#define MSE_EP_HD inline
#endif

namespace mseep {

constexpr int kEpisodeChunk = 8; // steps whose loads are issued together
constexpr int kTotals = 5;       // totals[]: counted episodes, sum return, sum length, min return, max return
constexpr int kSummary = 6;      // summary[]: episodes, mean return, std return, mean length, min, max

// counts and lengths are kept in double: integers below 2^53 add exactly in any order
struct Totals {
    double count, sum_return, sum_length, min_return, max_return;
};

MSE_EP_HD Totals totals_identity() { return Totals{0.0, 0.0, 0.0, (double)INFINITY, -(double)INFINITY}; }

// a (+) b: sums added as a + b, min / max by comparison (never NaN-propagating surprises: returns are finite sums)
MSE_EP_HD Totals totals_merge(const Totals &a, const Totals &b)
{
    return Totals{a.count + b.count, a.sum_return + b.sum_return, a.sum_length + b.sum_length,
                  b.min_return < a.min_return ? b.min_return : a.min_return, b.max_return > a.max_return ? b.max_return : a.max_return};
}

// totals[] (+)= t.  The caller's min / max count only if its own episode count is positive, so a zero-filled totals[]
// is the empty window; a call that counted nothing leaves all five cells as they were.
MSE_EP_HD void totals_fold_into(double *totals, const Totals &t)
{
    if (!(t.count > 0.0)) return;
    const bool had = totals[0] > 0.0;
    const double mn = had && totals[3] < t.min_return ? totals[3] : t.min_return;
    const double mx = had && totals[4] > t.max_return ? totals[4] : t.max_return;
    totals[0] = totals[0] + t.count;
    totals[1] = totals[1] + t.sum_return;
    totals[2] = totals[2] + t.sum_length;
    totals[3] = mn;
    totals[4] = mx;
}

struct WalkArgs {
    int k_steps;
    long long n;
    const float *rewards;          // f32[K, N]
    const uint8_t *dones;          // u8[K, N], or NULL with the two below
    const uint8_t *episode_starts; // u8[K, N]
    const uint8_t *last_dones;     // u8[N]
    double *run_return;            // f64[N] carry
    int32_t *run_length;           // i32[N] carry
    int32_t *ep_count;             // i32[N]
    const int32_t *targets;        // i32[N] or NULL
    int slots;                     // E, 0 without a ledger
    double *ledger_return;         // f64[E, N] or NULL
    int32_t *ledger_length;        // i32[E, N] or NULL
};

struct WalkState {
    double ret;
    int len, cnt;
};

MSE_EP_HD uint8_t end_mark(const WalkArgs &a, int k, long long i)
{
    if (a.dones != nullptr) return a.dones[(long long)k * a.n + i];
    return k + 1 < a.k_steps ? a.episode_starts[(long long)(k + 1) * a.n + i] : a.last_dones[i];
}

MSE_EP_HD void walk_step(const WalkArgs &a, long long i, int target, bool limited, float r, uint8_t ended, WalkState &s, Totals &t)
{
    s.ret = s.ret + (double)r;
    s.len = s.len + 1;
    if (ended != 0) {
        if (!limited || s.cnt < target) {
            if (a.ledger_return != nullptr && s.cnt < a.slots) {
                a.ledger_return[(long long)s.cnt * a.n + i] = s.ret;
                a.ledger_length[(long long)s.cnt * a.n + i] = s.len;
            }
            t.count = t.count + 1.0;
            t.sum_return = t.sum_return + s.ret;
            t.sum_length = t.sum_length + (double)s.len;
            t.min_return = s.ret < t.min_return ? s.ret : t.min_return;
            t.max_return = s.ret > t.max_return ? s.ret : t.max_return;
            s.cnt = s.cnt + 1;
        }
        s.ret = 0.0;
        s.len = 0;
    }
}

// the walk of env i; its counted episodes are merged into t in the order they end
MSE_EP_HD void episode_walk(const WalkArgs &a, long long i, Totals &t)
{
    WalkState s{a.run_return[i], a.run_length[i], a.ep_count[i]};
    const bool limited = a.targets != nullptr;
    const int target = limited ? a.targets[i] : 0;
    int k = 0;
    for (; k + kEpisodeChunk <= a.k_steps; k += kEpisodeChunk) {
        float r[kEpisodeChunk];
        uint8_t e[kEpisodeChunk];
#pragma unroll
        for (int j = 0; j < kEpisodeChunk; ++j) {
            r[j] = a.rewards[(long long)(k + j) * a.n + i];
            e[j] = end_mark(a, k + j, i);
        }
#pragma unroll
        for (int j = 0; j < kEpisodeChunk; ++j) walk_step(a, i, target, limited, r[j], e[j], s, t);
    }
    for (; k < a.k_steps; ++k) walk_step(a, i, target, limited, a.rewards[(long long)k * a.n + i], end_mark(a, k, i), s, t);
    a.run_return[i] = s.ret;
    a.run_length[i] = s.len;
    a.ep_count[i] = s.cnt;
}

// ---- summary ----------------------------------------------------------------------------------------------------------
// the counted ledger entries of env i are slots 0 .. min(ep_count[i], slots) - 1
MSE_EP_HD int ledger_entries(const int32_t *ep_count, int slots, long long i)
{
    const int c = ep_count[i];
    return c < 0 ? 0 : (c < slots ? c : slots);
}

MSE_EP_HD void summary_pass1(long long n, int slots, const int32_t *ep_count, const double *ledger_return,
                             const int32_t *ledger_length, long long i, Totals &t)
{
    const int m = ledger_entries(ep_count, slots, i);
    for (int e = 0; e < m; ++e) {
        const double x = ledger_return[(long long)e * n + i];
        t.count = t.count + 1.0;
        t.sum_return = t.sum_return + x;
        t.sum_length = t.sum_length + (double)ledger_length[(long long)e * n + i];
        t.min_return = x < t.min_return ? x : t.min_return;
        t.max_return = x > t.max_return ? x : t.max_return;
    }
}

MSE_EP_HD double summary_pass2(long long n, int slots, const int32_t *ep_count, const double *ledger_return, long long i,
                               double mean, double q)
{
    const int m = ledger_entries(ep_count, slots, i);
    for (int e = 0; e < m; ++e) {
        const double d = ledger_return[(long long)e * n + i] - mean;
        q = q + d * d;
    }
    return q;
}

MSE_EP_HD double summary_mean(const Totals &t) { return t.count > 0.0 ? t.sum_return / t.count : (double)NAN; }

MSE_EP_HD void summary_finish(const Totals &t, double mean, double q, double *summary)
{
    const bool any = t.count > 0.0;
    summary[0] = t.count;
    summary[1] = mean;
    summary[2] = any ? sqrt(q / t.count) : (double)NAN;
    summary[3] = any ? t.sum_length / t.count : (double)NAN;
    summary[4] = any ? t.min_return : (double)NAN;
    summary[5] = any ? t.max_return : (double)NAN;
}

} // namespace mseep
