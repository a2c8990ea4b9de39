// mse_ppo_matrix.h -- what mse_ppo.hip (the C ABI, k_ppo_adv_partial, k_ppo_reduce) and mse_ppo_matrix.hip (the
// matrix-core gradient kernel) share: the kernel's arguments, its grid rule and its launcher.  Host code only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mse_ppo_math.h"

struct MsePpoMatrixArgs {
    int D, A;
    long long n_rows, batch;
    int n_adv_partial;     // 0: advantages are used as they are
    mseppo::Params P;
    long long slab_stride; // floats between two workgroups' slabs
    int gate_cell;         // statistics cell of slab 0 in which workgroup 0 leaves the gate it saw
};

// rows a workgroup takes per pass of its grid-stride loop: two tile slots of 64 rows
constexpr int kMsePpoMatrixRowsPerGroup = 128;

// workgroups for `batch` rows on a device of `cus` compute units: one per 128 rows, at most two per CU and max_slabs
static inline long long mse_ppo_matrix_groups(long long batch, int cus, int max_slabs)
{
    long long n = (batch + kMsePpoMatrixRowsPerGroup - 1) / kMsePpoMatrixRowsPerGroup;
    const long long cap = 2LL * cus < max_slabs ? 2LL * cus : max_slabs;
    return n > cap ? cap : n;
}

// Enqueues k_ppo_grad_matrix on `n_slabs` workgroups; writes what k_ppo_grad writes: one slab of W + 8 floats per
// workgroup.  Returns hipSuccess or the error that kept the kernel from being launched.
hipError_t mse_ppo_launch_grad_matrix(const MsePpoMatrixArgs &G, int n_slabs, hipStream_t stream, const float *weights,
                                      const long long *rows, const float *obs, const uint8_t *mask, const int *actions,
                                      const float *old_logp, const float *adv, const float *ret, const double *adv_partial,
                                      float *slabs, const int *control);
