// mse_ppo_grad.h -- what the two forms of the learner's gradient launch share: k_ppo_grad (mse_ppo.hip, fmaf chains) and
// k_ppo_grad_matrix (mse_ppo_matrix.hip, matrix cores), and the kernels that run around either (k_ppo_adv_partial,
// k_ppo_reduce).  The slab protocol, the kernel arguments, the grid rule, the device helpers and what of a gradient kernel's
// frame can live in a helper are defined here once; the tile-loop bodies are the two forms and stay in their files.
// DESIGN.md 4.12.  HIP only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "mse_ppo_math.h"

namespace mseppo {

// ---- the slab protocol ----------------------------------------------------------------------------------------------------
// A workgroup of a gradient kernel stores ONE slab into the workspace: the W floats of its gradient in the flat order of
// include/mse.h, then kStatFloats floats of statistics (sums over the workgroup's rows; k_ppo_reduce divides by the batch):
//   0 surrogate   1 squared value error   2 entropy   3 kl   4 clipped   5 the gate cell (slab 0 only)   6, 7 zero
// k_ppo_reduce sums the slabs in slab order in double.  The behaviour-cloning instantiations (BC, mse_bc_loss_grad) keep the
// protocol and fill the same cells with their own sums, so k_ppo_reduce serves them as it stands:
//   0 cross-entropy   1 squared value error   2 entropy   3 hits   4 unusable rows   5 the gate cell, always 0   6, 7 zero
constexpr int kMaxSlabs = 512; // workgroups of a gradient kernel at most (two per CU on 256 CUs)
constexpr int kStatFloats = 8;
constexpr int kStatSums = 5; // cells 0 .. 4 are sums
// control = {stopped, minibatches_run} (caller-owned, NULL: no gate).  Only the lane of k_ppo_reduce that writes stats_out
// ever writes it, so a kernel that reads `stopped` at entry reads what an EARLIER launch of the stream left: the load
// is uniform over the whole grid.  k_ppo_reduce itself cannot read it that way (its other workgroups may start after
// that lane has stored), so workgroup 0 of the gradient kernel, one launch earlier, leaves the value it saw in this cell of
// slab 0's statistics (a cell no sum reads; 0 when there is no gate, as it always was) and k_ppo_reduce gates on that.
constexpr int kGateCell = 5;

__host__ __device__ constexpr long long slab_stride(long long w) { return (w + kStatFloats + 3) / 4 * 4; }

// The KICK instantiations (PPO with an imitation term, mse_ppo_bc_loss_grad) carry three more sums than the slab has free cells,
// so THEIR slabs are four floats wider: cells 0 .. 7 as above, then
//   8 cross-entropy of the label   9 hits   10 unusable rows   11 zero
// and their workspace is sized by mse_ppo_bc_workspace_bytes.  The other kernels' slabs are as they were.
constexpr int kKickStatFloats = 12;
constexpr int kKickCe = 8; // first of the three
__host__ __device__ constexpr long long slab_stride_kick(long long w) { return (w + kKickStatFloats + 3) / 4 * 4; }

// rows a workgroup takes per pass of its grid-stride loop: two tile slots of 64 rows.  Used by the host rule below only: the
// kernels' tile loops state the two slots and the 64 rows themselves (tile = 2 blockIdx.x + (wave >> 1), row = 64 tile + lane)
constexpr int kRowsPerGroup = 128;

// workgroups (= slabs) for `batch` rows on a device of `cus` compute units: one per 128 rows, at most two per CU
inline long long grad_groups(long long batch, int cus)
{
    const long long n = (batch + kRowsPerGroup - 1) / kRowsPerGroup;
    const long long cap = 2LL * cus < kMaxSlabs ? 2LL * cus : kMaxSlabs;
    return n > cap ? cap : n;
}

struct GradArgs {
    int D, A;
    long long n_rows, batch;
    int n_adv_partial; // 0: advantages are used as they are
    Params P;
};

// The end of a gradient kernel's dynamic LDS, behind its weight image and its four strips (no static __shared__: it would
// shift the dynamic base off its 16-byte alignment): [0] advantage mean, [1] std, [4 + 4 w + k] loss sum k of wave w
constexpr int kMiscFloats = 20;

// ---- device helpers -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool gate_closed(const int *control) { return control != nullptr && control[0] != 0; }

__device__ __forceinline__ long long row_at(const long long *rows, long long b, long long n_rows)
{
    long long r = rows == nullptr ? b : rows[b];
    r = r < 0 ? 0 : r;
    return r >= n_rows ? n_rows - 1 : r; // an index outside the rollout is clamped, never followed
}

// mean and unbiased std from k_ppo_adv_partial's partials, summed in index order (every caller gets the same bits)
__device__ __forceinline__ void adv_mean_std(const double *partial, int n_partial, double pivot, long long batch, float &mean, float &std)
{
    double s = 0.0, q = 0.0;
    for (int g = 0; g < n_partial; ++g) {
        s += partial[2 * g];
        q += partial[2 * g + 1];
    }
    const double var = (q - s * s / (double)batch) / (double)(batch - 1);
    mean = (float)(pivot + s / (double)batch);
    std = (float)sqrt(var > 0.0 ? var : 0.0);
}

__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64); // fixed butterfly
    return v;
}

// ---- the frame of a gradient kernel -----------------------------------------------------------------------------------------
// Each of these leaves k_ppo_grad's instructions as they were without it (tools/same_isa.py).  The rest of the frame stays in
// the two kernels because no helper form did: the legal-action word and policy_head_terms with the four sums (either as a
// helper reorders the tile loop), and the slot exchange (4 bias registers per layer against 1).
// the mark for k_ppo_reduce: all a closed gate writes (w_total = flat_layout(D, A).total; passing GradArgs moves instructions)
__device__ __forceinline__ void mark_gate_closed(int w_total, float *slabs)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) slabs[w_total + kGateCell] = 1.0f;
}

// wave 0 leaves the advantage mean and std in misc[0], misc[1]; the caller's __syncthreads publishes them
__device__ __forceinline__ void publish_adv_mean_std(const GradArgs &G, const long long *rows, const float *adv,
                                                     const double *adv_partial, float *misc, int wave, int lane)
{
    if (wave == 0) { // every lane sums the same partials in the same order
        float mean = 0.0f, std = 1.0f;
        if (G.n_adv_partial > 0) adv_mean_std(adv_partial, G.n_adv_partial, (double)adv[row_at(rows, 0, G.n_rows)], G.batch, mean, std);
        if (lane == 0) {
            misc[0] = mean;
            misc[1] = std;
        }
    }
}

// ---- a minibatch whose rows live in several places (mse_ppo_shard_*) -----------------------------------------
// What a SHARD instantiation reads beyond the other kernels' arguments; {0, NULL} for those, which never read it.  In a SHARD
// launch G.batch is the LOCAL row count (the tile loop's bound), every per-row term is scaled by 1 / global_batch, and
// G.n_adv_partial is only a flag (0 or 1): the mean and std come from `moments`, not from k_ppo_adv_partial's partials.
struct ShardArgs {
    long long global_batch; // B: rows of the minibatch over all shards
    const double *moments;  // f64[4]: {count, sum a, sum a^2, 0} over all shards
};

// the shard partial: W gradient sums, kStatSums statistic sums (not divided), padding to a multiple of 4; all double
__host__ __device__ constexpr long long shard_partial_len(long long w) { return (w + kStatSums + 3) / 4 * 4; }

// mean and unbiased std of the whole minibatch from its moments; every caller gets the same bits
__device__ __forceinline__ void shard_mean_std(const double *moments, long long batch, float &mean, float &std)
{
    const double s = moments[1], q = moments[2];
    const double var = (q - s * s / (double)batch) / (double)(batch - 1);
    mean = (float)(s / (double)batch);
    std = (float)sqrt(var > 0.0 ? var : 0.0);
}

// publish_adv_mean_std of a SHARD instantiation
__device__ __forceinline__ void publish_shard_mean_std(const GradArgs &G, const ShardArgs &S, float *misc, int wave, int lane)
{
    if (wave == 0) {
        float mean = 0.0f, std = 1.0f;
        if (G.n_adv_partial > 0) shard_mean_std(S.moments, S.global_batch, mean, std);
        if (lane == 0) {
            misc[0] = mean;
            misc[1] = std;
        }
    }
}

// an action outside the head is clamped into it, never followed
__device__ __forceinline__ int clamped_action(int action, int A) { return action < 0 ? 0 : (action >= A ? A - 1 : action); }

// a wave's four loss sums (already summed over its lanes; the actor's surrogate, entropy, kl, clipped, the critic's squared
// error in s0) into misc; the caller's __syncthreads publishes them
__device__ __forceinline__ void publish_loss_sums(float *misc, int wave, int lane, float s0, float s1, float s2, float s3)
{
    if (lane == 0) {
        float *s = misc + 4 + 4 * wave;
        s[0] = s0;
        s[1] = s1;
        s[2] = s2;
        s[3] = s3;
    }
}

// the statistics cells of a slab from the four waves' sums: actor waves 0 and 2, critic waves 1 and 3, slot 0 + slot 1
__device__ __forceinline__ void store_slab_stats(float *s, const float *misc)
{
    const float(*sh)[4] = reinterpret_cast<const float(*)[4]>(misc + 4);
    s[0] = sh[0][0] + sh[2][0]; // surrogate
    s[1] = sh[1][0] + sh[3][0]; // squared value error
    s[2] = sh[0][1] + sh[2][1]; // entropy
    s[3] = sh[0][2] + sh[2][2]; // kl
    s[4] = sh[0][3] + sh[2][3]; // clipped
    s[5] = s[6] = s[7] = 0.0f;
}

// ... and of a KICK instantiation, whose actor waves carry seven sums (the four above, then ce, hits, unusable): its misc
// strip is kKickMiscFloats long, [0] and [1] as above, [4 + 8 w + k] loss sum k of wave w
constexpr int kKickMiscFloats = 36;

__device__ __forceinline__ void publish_loss_sums_kick(float *misc, int wave, int lane, const float (&sum)[7])
{
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 7; ++k) misc[4 + 8 * wave + k] = sum[k];
    }
}

// cells 0 .. 7 are store_slab_stats' with the same additions; s has kKickStatFloats cells
__device__ __forceinline__ void store_slab_stats_kick(float *s, const float *misc)
{
    const float(*sh)[8] = reinterpret_cast<const float(*)[8]>(misc + 4);
    s[0] = sh[0][0] + sh[2][0]; // surrogate
    s[1] = sh[1][0] + sh[3][0]; // squared value error
    s[2] = sh[0][1] + sh[2][1]; // entropy
    s[3] = sh[0][2] + sh[2][2]; // kl
    s[4] = sh[0][3] + sh[2][3]; // clipped
    s[5] = s[6] = s[7] = 0.0f;
    s[kKickCe] = sh[0][4] + sh[2][4];     // cross-entropy of the label
    s[kKickCe + 1] = sh[0][5] + sh[2][5]; // hits
    s[kKickCe + 2] = sh[0][6] + sh[2][6]; // unusable rows
    s[kKickCe + 3] = 0.0f;
}

// what a KICK instantiation reads beyond the other kernels' arguments; {NULL, 0} for those, which never read it
struct KickArgs {
    const int *expert_actions; // i32[n_rows]: the label of every row
    float bc_coef;
};

} // namespace mseppo

// mse_ppo_matrix.hip: enqueues k_ppo_grad_matrix on `n_slabs` workgroups; it writes what k_ppo_grad writes.  Returns
// hipSuccess or the error that kept the kernel from being launched.
// old_values (f32[n_rows] or NULL), here and in launch_grad of mse_ppo.hip: non-NULL launches the VCLIP = true instantiation
// of the kernel, whose critic reads old_values at the row it reads `ret` at and calls value_head_terms_clipped with
// G.P.clip_range_vf; NULL launches VCLIP = false, which never reads the argument and is the kernel as it was without it.
hipError_t mse_ppo_launch_grad_matrix(const mseppo::GradArgs &G, int n_slabs, hipStream_t stream, const float *weights,
                                      const long long *rows, const float *obs, const uint8_t *mask, const int *actions,
                                      const float *old_logp, const float *adv, const float *ret, const double *adv_partial,
                                      float *slabs, const int *control, const float *old_values);
// ... the SHARD entry (mse_ppo_shard_loss_grad): G.batch local rows, terms scaled by 1 / S.global_batch, mean and std from
// S.moments; it writes what k_ppo_grad_shard writes
hipError_t mse_ppo_launch_grad_matrix_shard(const mseppo::GradArgs &G, int n_slabs, hipStream_t stream, const float *weights,
                                            const long long *rows, const float *obs, const uint8_t *mask, const int *actions,
                                            const float *old_logp, const float *adv, const float *ret, float *slabs,
                                            const int *control, const float *old_values, const mseppo::ShardArgs &S);
// ... the BC instantiation of k_ppo_grad_matrix (behaviour cloning: `actions` are the demonstrated ones; ret may be NULL, the
// critic then takes no tile); it writes what the BC instantiation of k_ppo_grad writes
hipError_t mse_ppo_launch_grad_matrix_bc(const mseppo::GradArgs &G, int n_slabs, hipStream_t stream, const float *weights,
                                         const long long *rows, const float *obs, const uint8_t *mask, const int *actions,
                                         const float *ret, float *slabs);
// ... the KICK entry (PPO with an imitation term on K.expert_actions); it writes what k_ppo_grad_kick writes
hipError_t mse_ppo_launch_grad_matrix_kick(const mseppo::GradArgs &G, int n_slabs, hipStream_t stream, const float *weights,
                                           const long long *rows, const float *obs, const uint8_t *mask, const int *actions,
                                           const float *old_logp, const float *adv, const float *ret, const double *adv_partial,
                                           float *slabs, const int *control, const float *old_values, const mseppo::KickArgs &K);
