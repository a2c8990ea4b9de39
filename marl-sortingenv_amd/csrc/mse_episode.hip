// Episode accounting on the device: cumulative reward and length per episode out of step-major rollout buffers
// (mse_episode_scan), mean / std over the recorded episodes (mse_episode_summary), and their host twins.  The per-env
// arithmetic lives in mse_episode_math.h (host + device); this file holds the kernels and the C ABI.  gfx950 only.
//
// k_episode_scan, DESIGN.md 4.13.  One env per lane, 256 lanes per workgroup, a grid-stride loop over blocks of 256
// envs: lane t of workgroup b walks envs 256 (b + j G) + t, j = 0, 1, .., for a grid of G workgroups,
// G = min(ceil(N / 256), kGroupsPerCu x CUs, kMaxSlabs) - a fixed function of N and the device.  The walk is a
// 5 B/row stream (reward f32 + end mark u8, both coalesced over the lanes) with a loop-carried double add; the loads of
// eight steps are issued before the adds that use them.  A lane merges its counted episodes into five doubles in
// (env, step) order; the wave reduces them with 6 shuffle steps (lane l takes lane l + 32, 16, .., 1), wave 0 .. 3 are
// added in that order through LDS, and the workgroup stores ONE slab of five doubles into the workspace.
// k_episode_fold (one workgroup) gives slab s to lane s mod 256, a lane adds its slabs in ascending order, the same
// wave / LDS reduction follows and lane 0 folds the result into totals[].  No atomics anywhere: same inputs, same bits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "mse.h"
#include "mse_host.h"
#include "mse_episode_math.h"

namespace {

using namespace mseep;

constexpr int kLanes = 256;      // per workgroup, four waves
constexpr int kGroupsPerCu = 4;  // the grid cap: 16 waves per CU
constexpr int kMaxSlabs = 1024;  // workgroups of k_episode_scan at most = slabs in the workspace
constexpr size_t kReduceLds = (kLanes / 64) * kTotals * sizeof(double);

extern __shared__ __attribute__((aligned(16))) char ep_lds[];

__device__ __forceinline__ Totals wave_reduce(Totals t)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        Totals o;
        o.count = __shfl_down(t.count, off, 64);
        o.sum_return = __shfl_down(t.sum_return, off, 64);
        o.sum_length = __shfl_down(t.sum_length, off, 64);
        o.min_return = __shfl_down(t.min_return, off, 64);
        o.max_return = __shfl_down(t.max_return, off, 64);
        t = totals_merge(t, o); // lanes whose partner lies past the wave merge their own copy: lane 0 never reads them
    }
    return t;
}

// the workgroup's Totals, valid in thread 0: waves in ascending order
__device__ __forceinline__ Totals group_reduce(Totals t)
{
    double *part = reinterpret_cast<double *>(ep_lds);
    t = wave_reduce(t);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        part[wave * kTotals + 0] = t.count;
        part[wave * kTotals + 1] = t.sum_return;
        part[wave * kTotals + 2] = t.sum_length;
        part[wave * kTotals + 3] = t.min_return;
        part[wave * kTotals + 4] = t.max_return;
    }
    __syncthreads();
    Totals g = totals_identity();
    if (threadIdx.x == 0) {
        for (int w = 0; w < kLanes / 64; ++w)
            g = totals_merge(g, Totals{part[w * kTotals + 0], part[w * kTotals + 1], part[w * kTotals + 2], part[w * kTotals + 3],
                                       part[w * kTotals + 4]});
    }
    return g;
}

__global__ __launch_bounds__(kLanes) void k_episode_scan(WalkArgs a, double *__restrict__ slabs)
{
    Totals t = totals_identity();
    const long long stride = (long long)gridDim.x * kLanes;
    for (long long i = (long long)blockIdx.x * kLanes + threadIdx.x; i < a.n; i += stride) episode_walk(a, i, t);
    if (slabs == nullptr) return; // uniform: no totals were asked for
    const Totals g = group_reduce(t);
    if (threadIdx.x == 0) {
        double *slab = slabs + (long long)blockIdx.x * kTotals;
        slab[0] = g.count;
        slab[1] = g.sum_return;
        slab[2] = g.sum_length;
        slab[3] = g.min_return;
        slab[4] = g.max_return;
    }
}

__global__ __launch_bounds__(kLanes) void k_episode_fold(int n_slabs, const double *__restrict__ slabs, double *__restrict__ totals)
{
    Totals t = totals_identity();
    for (int s = threadIdx.x; s < n_slabs; s += kLanes) {
        const double *slab = slabs + (long long)s * kTotals;
        t = totals_merge(t, Totals{slab[0], slab[1], slab[2], slab[3], slab[4]});
    }
    const Totals g = group_reduce(t);
    if (threadIdx.x == 0) totals_fold_into(totals, g);
}

// one workgroup: lane t takes envs t, t + 256, ..; both passes use the same reduction as the scan
__global__ __launch_bounds__(kLanes) void k_episode_summary(long long n, int slots, const int32_t *__restrict__ ep_count,
                                                            const double *__restrict__ ledger_return,
                                                            const int32_t *__restrict__ ledger_length, double *__restrict__ summary)
{
    double *share = reinterpret_cast<double *>(ep_lds) + (kLanes / 64) * kTotals; // the mean, for all lanes
    Totals t = totals_identity();
    for (long long i = threadIdx.x; i < n; i += kLanes) summary_pass1(n, slots, ep_count, ledger_return, ledger_length, i, t);
    const Totals g = group_reduce(t);
    if (threadIdx.x == 0) share[0] = summary_mean(g);
    __syncthreads();
    const double mean = share[0];
    double q = 0.0;
    for (long long i = threadIdx.x; i < n; i += kLanes) q = summary_pass2(n, slots, ep_count, ledger_return, i, mean, q);
    Totals tq = totals_identity();
    tq.sum_return = q; // thread 0 has read the partials of pass 1 before the barrier above
    const Totals gq = group_reduce(tq);
    if (threadIdx.x == 0) summary_finish(g, mean, gq.sum_return, summary);
}

// the argument rules of both scan entry points; nullptr if they hold
const char *scan_args_error(int32_t k_steps, int64_t n, const float *rewards, const uint8_t *dones, const uint8_t *episode_starts,
                            const uint8_t *last_dones, const double *run_return, const int32_t *run_length, const int32_t *ep_count,
                            int32_t slots, const double *ledger_return, const int32_t *ledger_length)
{
    if (k_steps < 1 || n < 1) return "k_steps and n must be positive";
    if (rewards == nullptr || run_return == nullptr || run_length == nullptr || ep_count == nullptr)
        return "rewards, run_return, run_length and ep_count must be given";
    const bool starts_form = episode_starts != nullptr && last_dones != nullptr;
    const bool starts_any = episode_starts != nullptr || last_dones != nullptr;
    if ((dones != nullptr) == starts_any || (starts_any && !starts_form))
        return "give either dones, or episode_starts with last_dones";
    if ((ledger_return == nullptr) != (ledger_length == nullptr)) return "ledger_return and ledger_length go together";
    if (slots < 0 || (ledger_return != nullptr) != (slots > 0)) return "slots must be positive with a ledger and 0 without";
    return nullptr;
}

const char *summary_args_error(int64_t n, int32_t slots, const int32_t *ep_count, const double *ledger_return,
                               const int32_t *ledger_length, const double *summary)
{
    if (ledger_return == nullptr || ledger_length == nullptr || slots < 1) return "a summary needs a ledger (slots >= 1)";
    if (n < 1) return "n must be positive";
    if (ep_count == nullptr || summary == nullptr) return "null argument";
    return nullptr;
}

bool misaligned8(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7u) != 0; }

} // namespace

extern "C" {

int64_t mse_episode_workspace_bytes(void) { return (int64_t)(kMaxSlabs * kTotals * sizeof(double)); }

int mse_episode_scan(int32_t k_steps, int64_t n, const float *rewards, const uint8_t *dones, const uint8_t *episode_starts,
                     const uint8_t *last_dones, double *run_return, int32_t *run_length, int32_t *ep_count, const int32_t *targets,
                     int32_t slots, double *ledger_return, int32_t *ledger_length, double *totals, void *workspace, void *stream)
{
    if (const char *why = scan_args_error(k_steps, n, rewards, dones, episode_starts, last_dones, run_return, run_length, ep_count,
                                          slots, ledger_return, ledger_length))
        return mse_internal_fail(MSE_ERR_INVALID_ARGUMENT, (std::string("mse_episode_scan: ") + why).c_str());
    if (totals != nullptr && workspace == nullptr)
        return mse_internal_fail(MSE_ERR_INVALID_ARGUMENT, "mse_episode_scan: totals need a workspace");
    if (misaligned8(run_return) || misaligned8(ledger_return) || misaligned8(totals) || misaligned8(workspace))
        return mse_internal_fail(MSE_ERR_ALIGNMENT, "mse_episode_scan: the double arrays must be 8-byte aligned");
    const int cus = cu_count();
    if (cus <= 0) return mse_internal_fail(MSE_ERR_NO_DEVICE, "mse_episode_scan: no HIP device (mse_episode_scan_host runs on the CPU)");
    long long groups = ((long long)n + kLanes - 1) / kLanes;
    const long long cap = (long long)kGroupsPerCu * cus < kMaxSlabs ? (long long)kGroupsPerCu * cus : kMaxSlabs;
    if (groups > cap) groups = cap;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const WalkArgs a{(int)k_steps, (long long)n, rewards, dones, episode_starts, last_dones, run_return, run_length, ep_count, targets,
                     (int)slots, ledger_return, ledger_length};
    double *slabs = totals == nullptr ? nullptr : static_cast<double *>(workspace);
    hipLaunchKernelGGL(k_episode_scan, dim3((unsigned)groups), dim3(kLanes), kReduceLds, s, a, slabs);
    if (totals != nullptr) hipLaunchKernelGGL(k_episode_fold, dim3(1), dim3(kLanes), kReduceLds, s, (int)groups, slabs, totals);
    if (hipGetLastError() != hipSuccess) return mse_internal_fail(MSE_ERR_HIP, "mse_episode_scan: kernel launch failed");
    return MSE_OK;
}

int mse_episode_scan_host(int32_t k_steps, int64_t n, const float *rewards, const uint8_t *dones, const uint8_t *episode_starts,
                          const uint8_t *last_dones, double *run_return, int32_t *run_length, int32_t *ep_count,
                          const int32_t *targets, int32_t slots, double *ledger_return, int32_t *ledger_length, double *totals)
{
    if (const char *why = scan_args_error(k_steps, n, rewards, dones, episode_starts, last_dones, run_return, run_length, ep_count,
                                          slots, ledger_return, ledger_length))
        return mse_internal_fail(MSE_ERR_INVALID_ARGUMENT, (std::string("mse_episode_scan_host: ") + why).c_str());
    const WalkArgs a{(int)k_steps, (long long)n, rewards, dones, episode_starts, last_dones, run_return, run_length, ep_count, targets,
                     (int)slots, ledger_return, ledger_length};
    Totals t = totals_identity();
    for (long long i = 0; i < (long long)n; ++i) episode_walk(a, i, t); // envs in ascending order
    if (totals != nullptr) totals_fold_into(totals, t);
    return MSE_OK;
}

int mse_episode_summary(int64_t n, int32_t slots, const int32_t *ep_count, const double *ledger_return, const int32_t *ledger_length,
                        double *summary, void *stream)
{
    if (const char *why = summary_args_error(n, slots, ep_count, ledger_return, ledger_length, summary))
        return mse_internal_fail(MSE_ERR_INVALID_ARGUMENT, (std::string("mse_episode_summary: ") + why).c_str());
    if (misaligned8(ledger_return) || misaligned8(summary))
        return mse_internal_fail(MSE_ERR_ALIGNMENT, "mse_episode_summary: the double arrays must be 8-byte aligned");
    if (cu_count() <= 0)
        return mse_internal_fail(MSE_ERR_NO_DEVICE, "mse_episode_summary: no HIP device (mse_episode_summary_host runs on the CPU)");
    hipLaunchKernelGGL(k_episode_summary, dim3(1), dim3(kLanes), kReduceLds + 2 * sizeof(double), static_cast<hipStream_t>(stream),
                       (long long)n, (int)slots, ep_count, ledger_return, ledger_length, summary);
    if (hipGetLastError() != hipSuccess) return mse_internal_fail(MSE_ERR_HIP, "mse_episode_summary: kernel launch failed");
    return MSE_OK;
}

int mse_episode_summary_host(int64_t n, int32_t slots, const int32_t *ep_count, const double *ledger_return,
                             const int32_t *ledger_length, double *summary)
{
    if (const char *why = summary_args_error(n, slots, ep_count, ledger_return, ledger_length, summary))
        return mse_internal_fail(MSE_ERR_INVALID_ARGUMENT, (std::string("mse_episode_summary_host: ") + why).c_str());
    Totals t = totals_identity();
    for (long long i = 0; i < (long long)n; ++i) summary_pass1(n, slots, ep_count, ledger_return, ledger_length, i, t);
    const double mean = summary_mean(t);
    double q = 0.0;
    for (long long i = 0; i < (long long)n; ++i) q = summary_pass2(n, slots, ep_count, ledger_return, i, mean, q);
    summary_finish(t, mean, q, summary);
    return MSE_OK;
}

} // extern "C"
