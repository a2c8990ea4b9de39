// Plant ledger on the device: per-episode plant quantities of every env out of all-env trace records (mse_plant_scan) and
// its host twin.  The per-env arithmetic lives in mse_plant_math.h (host + device); this file holds the kernels and the C
// ABI.  gfx950 only.
//
// k_plant_scan, DESIGN.md 4.21.  One env per lane, 256 lanes per workgroup, a grid-stride loop over blocks of 256 envs as in
// k_episode_scan: lane t of workgroup b walks envs 256 (b + j G) + t, j = 0, 1, .., G = min(ceil(N / 256), kGroupsPerCu x
// CUs, kMaxSlabs).  A step reads 20 of the record's 40 column planes (29 at an episode's end), each a run of consecutive
// doubles over the lanes, and carries 35 doubles.  A lane adds its counted episodes into 33 doubles in (env, step) order;
// the wave reduces them with 6 shuffle steps (lane l takes lane l + 32, 16, .., 1), the waves' partials meet in LDS where
// thread c adds cell c of wave 0 .. 3 in that order, and the workgroup stores ONE slab of 33 doubles into the workspace.
// k_plant_fold (one workgroup) gives slab s to lane s mod 256, a lane adds its slabs in ascending order, the same wave /
// LDS reduction follows and thread c adds cell c onto totals[c].  No atomics anywhere: same inputs, same bits.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "mse.h"
#include "mse_host.h"
#include "mse_plant_math.h"

static_assert(msepl::kCols == MSE_PLANT_COLS && msepl::kRunCols == MSE_PLANT_RUN_COLS && msepl::kRecCols == MSE_TRACE_COLS,
              "mse_plant_math.h and include/mse.h disagree");
static_assert(msepl::R_SORT == MSE_TRACE_R_SORT && msepl::R_PRESS == MSE_TRACE_R_PRESS && msepl::CONT_TRUE == MSE_TRACE_CONT_TRUE &&
                  msepl::CONT_FALSE == MSE_TRACE_CONT_FALSE && msepl::CONT_E == MSE_TRACE_CONT_E && msepl::N_LOG == MSE_TRACE_N_LOG &&
                  msepl::LOG == MSE_TRACE_LOG && msepl::N_BALE == MSE_TRACE_N_BALE && msepl::BALE == MSE_TRACE_BALE &&
                  msepl::DONE == MSE_TRACE_DONE && msepl::REWARD == MSE_TRACE_REWARD && msepl::OVERFLOW == MSE_TRACE_OVERFLOW,
              "mse_plant_math.h and include/mse.h disagree");

namespace {

using namespace msepl;

constexpr int kLanes = 256;      // per workgroup, four waves
constexpr int kWaves = kLanes / 64;
constexpr int kGroupsPerCu = 1;  // the grid cap: the walk holds 35 + 33 doubles per lane, one wave per SIMD is what fits
constexpr int kMaxSlabs = 1024;  // workgroups of k_plant_scan at most = slabs in the workspace
constexpr size_t kReduceLds = kWaves * kTotals * sizeof(double);

extern __shared__ __attribute__((aligned(16))) char plant_lds[];

// the workgroup's cell c, valid in thread c < kTotals: lanes by shuffle, then waves in ascending order
__device__ __forceinline__ double group_reduce(PlantTotals t)
{
    double *part = reinterpret_cast<double *>(plant_lds);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int c = 0; c < kTotals; ++c) t.v[c] = t.v[c] + __shfl_down(t.v[c], off, 64); // lanes past the wave add their own
                                                                                          // copy: lane 0 never reads them
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < kTotals; ++c) part[wave * kTotals + c] = t.v[c];
    }
    __syncthreads();
    double g = 0.0;
    if (threadIdx.x < kTotals) {
        for (int w = 0; w < kWaves; ++w) g = g + part[w * kTotals + threadIdx.x];
    }
    return g;
}

__global__ __launch_bounds__(kLanes) void k_plant_scan(PlantArgs a, double *__restrict__ slabs)
{
    PlantTotals t;
    totals_clear(t);
    const long long stride = (long long)gridDim.x * kLanes;
    for (long long i = (long long)blockIdx.x * kLanes + threadIdx.x; i < a.n; i += stride) plant_walk(a, i, t);
    if (slabs == nullptr) return; // uniform: no totals were asked for
    const double g = group_reduce(t);
    if (threadIdx.x < kTotals) slabs[(long long)blockIdx.x * kTotals + threadIdx.x] = g;
}

__global__ __launch_bounds__(kLanes) void k_plant_fold(int n_slabs, const double *__restrict__ slabs, double *__restrict__ totals)
{
    PlantTotals t;
    totals_clear(t);
    for (int s = threadIdx.x; s < n_slabs; s += kLanes) {
#pragma unroll
        for (int c = 0; c < kTotals; ++c) t.v[c] = t.v[c] + slabs[(long long)s * kTotals + c];
    }
    const double g = group_reduce(t);
    if (threadIdx.x < kTotals) totals[threadIdx.x] = totals[threadIdx.x] + g;
}

// the argument rules of both entry points, in the order include/mse.h documents; nullptr if they hold
const char *scan_args_error(int32_t k_steps, int64_t n, const double *records, int32_t S, int32_t U, const double *run,
                            const int32_t *ep_count, int32_t slots, const double *ledger)
{
    if (k_steps < 1 || n < 1) return "k_steps and n must be positive";
    if (records == nullptr || run == nullptr || ep_count == nullptr) return "records, run and ep_count must be given";
    if (slots < 0 || (ledger != nullptr) != (slots > 0)) return "slots must be positive with a ledger and 0 without";
    if (S < 1 || U < 0 || U >= S) return "bale_standard_size must be positive and 0 <= remainder_units < bale_standard_size";
    return nullptr;
}

bool misaligned8(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7u) != 0; }

} // namespace

extern "C" {

int64_t mse_plant_workspace_bytes(void) { return (int64_t)(kMaxSlabs * kTotals * sizeof(double)); }

int mse_plant_scan(int32_t k_steps, int64_t n, const double *records, int32_t bale_standard_size, int32_t remainder_units,
                   double *run, int32_t *ep_count, const int32_t *targets, int32_t slots, double *ledger, double *totals,
                   void *workspace, void *stream)
{
    if (const char *why = scan_args_error(k_steps, n, records, bale_standard_size, remainder_units, run, ep_count, slots, ledger))
        return mse_internal_fail(MSE_ERR_INVALID_ARGUMENT, (std::string("mse_plant_scan: ") + why).c_str());
    if (totals != nullptr && workspace == nullptr)
        return mse_internal_fail(MSE_ERR_INVALID_ARGUMENT, "mse_plant_scan: totals need a workspace");
    if (misaligned8(records) || misaligned8(run) || misaligned8(ledger) || misaligned8(totals) || misaligned8(workspace))
        return mse_internal_fail(MSE_ERR_ALIGNMENT, "mse_plant_scan: the double arrays must be 8-byte aligned");
    const int cus = cu_count();
    if (cus <= 0) return mse_internal_fail(MSE_ERR_NO_DEVICE, "mse_plant_scan: no HIP device (mse_plant_scan_host runs on the CPU)");
    long long groups = ((long long)n + kLanes - 1) / kLanes;
    const long long cap = (long long)kGroupsPerCu * cus < kMaxSlabs ? (long long)kGroupsPerCu * cus : kMaxSlabs;
    if (groups > cap) groups = cap;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const PlantArgs a{(int)k_steps, (long long)n, records, (int)bale_standard_size, (int)remainder_units, run, ep_count, targets,
                      (int)slots, ledger};
    double *slabs = totals == nullptr ? nullptr : static_cast<double *>(workspace);
    hipLaunchKernelGGL(k_plant_scan, dim3((unsigned)groups), dim3(kLanes), kReduceLds, s, a, slabs);
    if (totals != nullptr) hipLaunchKernelGGL(k_plant_fold, dim3(1), dim3(kLanes), kReduceLds, s, (int)groups, slabs, totals);
    if (hipGetLastError() != hipSuccess) return mse_internal_fail(MSE_ERR_HIP, "mse_plant_scan: kernel launch failed");
    return MSE_OK;
}

int mse_plant_scan_host(int32_t k_steps, int64_t n, const double *records, int32_t bale_standard_size, int32_t remainder_units,
                        double *run, int32_t *ep_count, const int32_t *targets, int32_t slots, double *ledger, double *totals)
{
    if (const char *why = scan_args_error(k_steps, n, records, bale_standard_size, remainder_units, run, ep_count, slots, ledger))
        return mse_internal_fail(MSE_ERR_INVALID_ARGUMENT, (std::string("mse_plant_scan_host: ") + why).c_str());
    if (misaligned8(records) || misaligned8(run) || misaligned8(ledger) || misaligned8(totals))
        return mse_internal_fail(MSE_ERR_ALIGNMENT, "mse_plant_scan_host: the double arrays must be 8-byte aligned");
    const PlantArgs a{(int)k_steps, (long long)n, records, (int)bale_standard_size, (int)remainder_units, run, ep_count, targets,
                      (int)slots, ledger};
    PlantTotals t;
    totals_clear(t);
    for (long long i = 0; i < (long long)n; ++i) plant_walk(a, i, t); // envs in ascending order
    if (totals != nullptr) {
        for (int c = 0; c < kTotals; ++c) totals[c] = totals[c] + t.v[c];
    }
    return MSE_OK;
}

} // extern "C"
