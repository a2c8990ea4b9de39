// mse_plant_math.h -- the plant ledger: per-episode plant quantities out of all-env trace records (mse_plant.hip), in
// plain C++ that compiles for the host and for the device alike (as mse_episode_math.h does): k_plant_scan and
// mse_plant_scan_host run plant_walk, so tests/test_plant_cpu.py can hold the arithmetic against tests/plant_reference.py
// without a GPU.
//
// What it restates: the reference's dashboard ledgers of ONE env - reward_data["Reward"] (r_sort, r_press) pairs
// (env_super.py:928-946), press_actions_per_timestep (:631-637, 730-736), the bale_count lists of press_bale (:661-687) and
// _calculate_avg_bale_deviation (:235-241) - folded into one row per episode, with the lists kept as O(1) sums.
//
// plant_walk, env column i of records f64[K, MSE_TRACE_COLS, N] (cell (k, c, i) at (k * 40 + c) * n + i), k = 0 .. K - 1:
//   1. the N_BALE (0..2) press_bale calls {material m, amount n, stored quality q} in order, on the per-material sums
//      cnt, mass, qsum, dev and the last bale's size `last` (S = bale_standard_size, U = remainder_units):
//        full = n / S, rem = n mod S  (integers)
//        full > 0:              cnt += full, mass += full S, qsum += full q, last = S              (|S - S| = 0)
//        rem > 0 and rem > U:   cnt += 1, mass += rem, qsum += q, dev += S - rem, last = rem      (a new short bale)
//        rem > 0, else cnt > 0: mass += rem, dev += |last + rem - S| - |last - S|, last += rem     (merged into the last bale,
//                                                                                                   which keeps its quality)
//        rem > 0, else:         cnt = 1, mass = rem, qsum = q, dev = S - rem, last = rem           (the episode's first bale)
//      n = 0 changes nothing.  This is the list form (trace.py:_press_bale): a merge replaces the last bale's |size - S|.
//   2. the N_LOG (0..2) press-log codes: 1 -> col 4, 2 -> col 5, 111 | 222 -> col 6, 0 -> col 7; any other code is ignored
//   3. length += 1; ret += REWARD, ret_sort += R_SORT, ret_press += R_PRESS: one double add each, in step order
//   4. DONE != 0 closes the episode: col 8 = OVERFLOW, col 9 = sum CONT_TRUE + sum CONT_FALSE + CONT_E of this record
//      (read only here).  The episode is COUNTED iff targets == NULL or ep_count[i] < targets[i]; a counted episode
//        - is stored, all MSE_PLANT_COLS cells (30, 31 zero), at ledger[ep_count[i], :, i] if a ledger is given and
//          0 <= ep_count[i] < slots,
//        - is added to the lane's totals: [0] += 1, [1 + c] += col c, col 8 as (overflow != 0),
//        - increments ep_count[i].
//      Counted or not, the carry (cols 0-29 and the five last sizes) is cleared.
// The carry run[c, i], c = 0 .. 34, is read before step 0 and written back after step K - 1 (cols 8, 9 as zeros; row 35 is
// not touched), so an episode spans any number of calls.  Every cell but cols 1-3 is an integer below 2^53 held in a double:
// those are exact whatever the order of the additions.  Cols 1-3 are sequential float64 sums in step order.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define MSE_PL_HD __host__ __device__ __forceinline__
#else
#define MSE_PL_HD inline
#endif

namespace msepl {

constexpr int kCols = 32;            // MSE_PLANT_COLS
constexpr int kRunCols = 36;         // MSE_PLANT_RUN_COLS
constexpr int kCarry = 35;           // rows of run[] in use: 30 columns + 5 last sizes
constexpr int kTotals = 1 + kCols;   // totals[]
constexpr int kRecCols = 40;         // MSE_TRACE_COLS
// the record columns read (include/mse.h MSE_TRACE_*)
constexpr int R_SORT = 1, R_PRESS = 2, CONT_TRUE = 8, CONT_FALSE = 12, CONT_E = 16, N_LOG = 17, LOG = 18, N_BALE = 22,
              BALE = 23, DONE = 29, REWARD = 32, OVERFLOW = 37;
// the row's columns
constexpr int C_LEN = 0, C_RET = 1, C_RSORT = 2, C_RPRESS = 3, C_P1 = 4, C_P2 = 5, C_BUSY = 6, C_NOOP = 7, C_OVF = 8,
              C_LEFT = 9, C_BALES = 10, C_MASS = 15, C_QSUM = 20, C_DEV = 25, C_LAST = 30;

struct PlantArgs {
    int k_steps;
    long long n;
    const double *records; // f64[K, 40, N]
    int S, U;              // bale_standard_size, remainder_units
    double *run;           // f64[36, N]
    int32_t *ep_count;     // i32[N]
    const int32_t *targets; // i32[N] or NULL
    int slots;
    double *ledger;        // f64[slots, 32, N] or NULL
};

struct PlantTotals {
    double v[kTotals];
};

MSE_PL_HD void totals_clear(PlantTotals &t)
{
#pragma unroll
    for (int c = 0; c < kTotals; ++c) t.v[c] = 0.0;
}

// the carry of one env: c[0..29] the row under construction, c[30..34] the last bale's size per material
struct PlantState {
    double c[kCarry];
};

MSE_PL_HD double abs_d(double x) { return x < 0.0 ? -x : x; }

// c[base + m] with m = 0..4 chosen by comparison, so the state stays in registers (no indexed access)
MSE_PL_HD double pick5(const PlantState &s, int base, int m)
{
    double x = s.c[base];
#pragma unroll
    for (int j = 1; j < 5; ++j) x = m == j ? s.c[base + j] : x;
    return x;
}
MSE_PL_HD void put5(PlantState &s, int base, int m, double x)
{
#pragma unroll
    for (int j = 0; j < 5; ++j) s.c[base + j] = m == j ? x : s.c[base + j];
}

MSE_PL_HD void press_bale(PlantState &s, int S, int U, int m, long long n, double q)
{
    if (m < 0 || m > 4 || n <= 0) return;
    const long long full = n / S;
    const int rem = (int)(n - full * S);
    double cnt = pick5(s, C_BALES, m), mass = pick5(s, C_MASS, m), qsum = pick5(s, C_QSUM, m), dev = pick5(s, C_DEV, m),
           last = pick5(s, C_LAST, m);
    const double dS = (double)S, drem = (double)rem;
    if (full > 0) {
        cnt = cnt + (double)full;
        mass = mass + (double)(full * S);
        qsum = qsum + (double)full * q;
        last = dS;
    }
    if (rem > 0) {
        if (rem > U) {
            cnt = cnt + 1.0;
            mass = mass + drem;
            qsum = qsum + q;
            dev = dev + (dS - drem);
            last = drem;
        } else if (cnt > 0.0) {
            mass = mass + drem;
            dev = dev + (abs_d(last + drem - dS) - abs_d(last - dS));
            last = last + drem;
        } else {
            cnt = 1.0;
            mass = drem;
            qsum = q;
            dev = dS - drem;
            last = drem;
        }
    }
    put5(s, C_BALES, m, cnt);
    put5(s, C_MASS, m, mass);
    put5(s, C_QSUM, m, qsum);
    put5(s, C_DEV, m, dev);
    put5(s, C_LAST, m, last);
}

MSE_PL_HD void press_code(PlantState &s, int code)
{
    s.c[C_P1] = s.c[C_P1] + (code == 1 ? 1.0 : 0.0);
    s.c[C_P2] = s.c[C_P2] + (code == 2 ? 1.0 : 0.0);
    s.c[C_BUSY] = s.c[C_BUSY] + ((code == 111 || code == 222) ? 1.0 : 0.0);
    s.c[C_NOOP] = s.c[C_NOOP] + (code == 0 ? 1.0 : 0.0);
}

// the walk of env i; its counted episodes are added to t in the order they end
MSE_PL_HD void plant_walk(const PlantArgs &a, long long i, PlantTotals &t)
{
    PlantState s;
#pragma unroll
    for (int c = 0; c < kCarry; ++c) s.c[c] = a.run[(long long)c * a.n + i];
    int cnt = a.ep_count[i];
    const bool limited = a.targets != nullptr;
    const int target = limited ? a.targets[i] : 0;
    for (int k = 0; k < a.k_steps; ++k) {
        const double *r = a.records + (long long)k * kRecCols * a.n + i; // column c at r[c * n]
        const long long n = a.n;
        // the loads of a step do not depend on the carry: take them first
        const double reward = r[REWARD * n], r_sort = r[R_SORT * n], r_press = r[R_PRESS * n], done = r[DONE * n];
        const int n_bale = (int)r[N_BALE * n], n_log = (int)r[N_LOG * n];
        const int code0 = (int)r[LOG * n], code1 = (int)r[(LOG + 2) * n];
        const int bm0 = (int)r[BALE * n], bm1 = (int)r[(BALE + 3) * n];
        const long long bn0 = (long long)r[(BALE + 1) * n], bn1 = (long long)r[(BALE + 4) * n];
        const double bq0 = r[(BALE + 2) * n], bq1 = r[(BALE + 5) * n];
        if (n_bale > 0) press_bale(s, a.S, a.U, bm0, bn0, bq0);
        if (n_bale > 1) press_bale(s, a.S, a.U, bm1, bn1, bq1);
        if (n_log > 0) press_code(s, code0);
        if (n_log > 1) press_code(s, code1);
        s.c[C_LEN] = s.c[C_LEN] + 1.0;
        s.c[C_RET] = s.c[C_RET] + reward;
        s.c[C_RSORT] = s.c[C_RSORT] + r_sort;
        s.c[C_RPRESS] = s.c[C_RPRESS] + r_press;
        if (done != 0.0) {
            double left = r[CONT_E * n];
#pragma unroll
            for (int m = 0; m < 4; ++m) left = left + r[(CONT_TRUE + m) * n] + r[(CONT_FALSE + m) * n];
            s.c[C_OVF] = r[OVERFLOW * n];
            s.c[C_LEFT] = left;
            if (!limited || cnt < target) {
                if (a.ledger != nullptr && cnt >= 0 && cnt < a.slots) {
                    double *row = a.ledger + (long long)cnt * kCols * a.n + i;
#pragma unroll
                    for (int c = 0; c < C_LAST; ++c) row[(long long)c * a.n] = s.c[c];
                    row[30LL * a.n] = 0.0;
                    row[31LL * a.n] = 0.0;
                }
                t.v[0] = t.v[0] + 1.0;
#pragma unroll
                for (int c = 0; c < C_LAST; ++c) t.v[1 + c] = t.v[1 + c] + (c == C_OVF ? (s.c[c] != 0.0 ? 1.0 : 0.0) : s.c[c]);
                cnt = cnt + 1;
            }
#pragma unroll
            for (int c = 0; c < kCarry; ++c) s.c[c] = 0.0;
        }
    }
#pragma unroll
    for (int c = 0; c < kCarry; ++c) a.run[(long long)c * a.n + i] = s.c[c];
    a.ep_count[i] = cnt;
}

} // namespace msepl
