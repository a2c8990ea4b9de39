// The second half of PPO on the device: returns and advantages (mse_gae), the clipped-surrogate loss of one minibatch
// with its gradient w.r.t. all weights (mse_ppo_loss_grad; with SB3's clip_range_vf, mse_ppo_loss_grad_vclip; the behaviour-
// cloning loss of demonstrated actions in the same kernels' BC instantiations, mse_bc_loss_grad; one minibatch whose rows live
// in several places as three phases around the SHARD instantiations, mse_ppo_shard_moments / _loss_grad / _finish), clip_grad_norm_
// + Adam (mse_ppo_adam_step), the counter-based permutation that orders an epoch's rows into minibatches (mse_ppo_shuffle, and
// its host twin) and SB3's train/explained_variance of a rollout (mse_explained_variance, and its host twin).  The
// per-row arithmetic lives in mse_ppo_math.h (host + device); this file holds the kernels and the C ABI.  gfx950 only.
//
// Gradient kernel (k_ppo_grad), DESIGN.md 4.12.  A workgroup is four waves: wave w works on the actor (w & 1 == 0) or
// the critic (w & 1 == 1) of tile slot w >> 1; a tile is 64 minibatch rows, one row per lane.  Per tile a wave
//   1. runs its network forward and backward for its row with plain fmaf chains, weights broadcast from LDS (padded
//      image, 16-byte reads), activations and deltas in registers;
//   2. per layer stages (delta, input activation) of 32 rows at a time in its own LDS strip and accumulates the weight
//      gradient  delta^T x activation  as a register-tiled product: lane (ob, ib) owns outputs 4 ob .. 4 ob + 3 times
//      inputs 4 ib .. 4 ib + 3 of every layer (16 accumulators + 4 bias sums per layer), rows are the k dimension.
// Accumulators stay in registers across all tiles of the wave.  At the end the two waves of a network are added in a
// fixed order through LDS and the workgroup stores ONE slab of W floats (+ 8 loss sums) into the workspace; k_ppo_reduce
// sums the slabs in slab order in double.  No atomics anywhere: same inputs, same bits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "mse.h"
#include "mse_host.h"
#include "mse_ppo_grad.h"
#include "mse_ppo_math.h"

namespace {

using namespace mseppo;

constexpr int kMaxAdvPartials = 256; // workgroups of k_ppo_adv_partial at most
constexpr int kStageStride = 68;     // floats per staged row: 32 deltas + 32 activations + 4 (16-byte rows, spread banks)
constexpr int kStageFloats = 32 * kStageStride;

// ---- the target_kl gate (mse_ppo_grad.h: kGateCell) -----------------------------------------------------------------------
struct Gate {
    int *control;    // NULL: no gate
    double kl_limit; // 1.5 * target_kl; <= 0: the flag is honoured and the count kept, but never set
};

// ---- GAE ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_gae(int k_steps, long long n, const float *__restrict__ rewards,
                                             const float *__restrict__ values, const uint8_t *__restrict__ episode_starts,
                                             const float *__restrict__ last_values, const uint8_t *__restrict__ last_dones,
                                             float g, float gl, float *__restrict__ adv_out, float *__restrict__ ret_out)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) gae_column(k_steps, n, i, rewards, values, episode_starts, last_values, last_dones, g, gl, adv_out, ret_out);
}

// ---- explained variance (mse_ppo_math.h specifies the sums and their order) ------------------------------------------------
// partial[4 g + k]: sum k of group g.  Every lane reads element 0 for the pivots (one broadcast line).
__global__ __launch_bounds__(256) void k_explained_variance_partial(long long n, const float *__restrict__ values,
                                                                    const float *__restrict__ returns, double *__restrict__ partial)
{
    __shared__ double sh[4][kEvLanes];
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    ev_lane_sums(n, (long long)blockIdx.x * kEvLanes + threadIdx.x, (long long)gridDim.x * kEvLanes, values, returns, acc);
#pragma unroll
    for (int k = 0; k < 4; ++k) sh[k][threadIdx.x] = acc[k];
    __syncthreads();
    for (int w = kEvLanes / 2; w > 0; w >>= 1) { // fixed tree
        if ((int)threadIdx.x < w) {
#pragma unroll
            for (int k = 0; k < 4; ++k) sh[k][threadIdx.x] += sh[k][threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x < 4) partial[4 * blockIdx.x + threadIdx.x] = sh[threadIdx.x][0];
}

// one lane adds the partials in index order and stores the one f32
__global__ __launch_bounds__(64) void k_explained_variance_finish(long long n, int groups, const double *__restrict__ partial,
                                                                  float *__restrict__ out)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double sums[4] = {0.0, 0.0, 0.0, 0.0};
    for (int g = 0; g < groups; ++g) {
#pragma unroll
        for (int k = 0; k < 4; ++k) sums[k] += partial[4 * g + k];
    }
    out[0] = (float)ev_from_sums(sums, n);
}

// the argument rules of both entry points; nullptr if they hold
const char *explained_variance_args_error(int64_t n, const float *values, const float *returns, const float *out)
{
    if (values == nullptr || returns == nullptr || out == nullptr) return "null argument";
    if (n < 1) return "n must be positive";
    return nullptr;
}

// ---- advantage mean / std: partial sums of d = a - pivot and d^2 in double, one pair per workgroup -------------------
__global__ __launch_bounds__(256) void k_ppo_adv_partial(long long batch, long long n_rows, const long long *__restrict__ rows,
                                                         const float *__restrict__ adv, double *__restrict__ partial,
                                                         const int *__restrict__ control)
{
    __shared__ double sh[2][256];
    if (gate_closed(control)) return;
    const double pivot = (double)adv[row_at(rows, 0, n_rows)];
    double s = 0.0, q = 0.0;
    for (long long b = (long long)blockIdx.x * 256 + threadIdx.x; b < batch; b += (long long)gridDim.x * 256) {
        const double d = (double)adv[row_at(rows, b, n_rows)] - pivot;
        s += d;
        q += d * d;
    }
    sh[0][threadIdx.x] = s;
    sh[1][threadIdx.x] = q;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) { // fixed tree
        if ((int)threadIdx.x < w) {
            sh[0][threadIdx.x] += sh[0][threadIdx.x + w];
            sh[1][threadIdx.x] += sh[1][threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = sh[0][0];
        partial[2 * blockIdx.x + 1] = sh[1][0];
    }
}

// ---- the gradient kernel ------------------------------------------------------------------------------------------------
template <int N>
__device__ __forceinline__ float padded_at(const float (&v)[N], int i) // i is a compile-time constant after unrolling
{
    return i < N ? v[i < N ? i : 0] : 0.0f;
}

// acc[4 p + q] += sum over the wave's 64 rows of delta[4 ob + p] * act[4 ib + q];  db[p] += sum of delta[4 ob + p].
// Rows go through the wave's LDS strip 32 at a time: [row][0..31] deltas, [row][32..63] activations.
template <int ND, int NA>
__device__ __forceinline__ void accumulate_layer(float *strip, int lane, const float (&delta)[ND], const float (&act)[NA],
                                                 float (&acc)[16], float (&db)[4])
{
    const int ob = lane >> 3, ib = lane & 7;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        if ((lane >> 5) == half) {
            float4 *dst = reinterpret_cast<float4 *>(strip + (lane & 31) * kStageStride);
#pragma unroll
            for (int c = 0; c < 8; ++c)
                dst[c] = make_float4(padded_at(delta, 4 * c), padded_at(delta, 4 * c + 1), padded_at(delta, 4 * c + 2), padded_at(delta, 4 * c + 3));
#pragma unroll
            for (int c = 0; c < 8; ++c)
                dst[8 + c] = make_float4(padded_at(act, 4 * c), padded_at(act, 4 * c + 1), padded_at(act, 4 * c + 2), padded_at(act, 4 * c + 3));
        }
        wave_lds_sync();
#pragma unroll 4
        for (int r = 0; r < 32; ++r) {
            const float4 d = *reinterpret_cast<const float4 *>(strip + r * kStageStride + 4 * ob);
            const float4 a = *reinterpret_cast<const float4 *>(strip + r * kStageStride + 32 + 4 * ib);
            const float dv[4] = {d.x, d.y, d.z, d.w}, av[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
            for (int p = 0; p < 4; ++p) {
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[4 * p + q] = fmaf(dv[p], av[q], acc[4 * p + q]);
                db[p] += dv[p];
            }
        }
        wave_lds_sync();
    }
}

struct LayerAcc {
    float w[16], b[4];
};

// one layer's accumulators -> the flat gradient: out[w_off + o * ld + i] (o < n_out, i < n_in), out[b_off + o]
__device__ __forceinline__ void store_layer(float *out, const LayerAcc &L, int lane, int w_off, int b_off, int n_out, int n_in, int ld)
{
    const int ob = lane >> 3, ib = lane & 7;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int o = 4 * ob + p;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = 4 * ib + q;
            if (o < n_out && i < n_in) out[w_off + o * ld + i] = L.w[4 * p + q];
        }
        if (ib == 0 && o < n_out) out[b_off + o] = L.b[p];
    }
}

// VCLIP: SB3's clip_range_vf (value_head_terms_clipped on old_values[row]); false never reads old_values
// BC: behaviour cloning (mse_bc_loss_grad).  The actor's head is bc_head_terms on actions[row], the demonstrated action, and
// its four sums are ce, entropy, hits, unusable rows (slab cells 0, 2, 3, 4); old_logp, adv and adv_partial are never read
// (G.n_adv_partial is 0).  The critic is value_head_terms on ret[row], or, with ret == NULL, takes no tile at all: its sums
// and its half of the slab are the zeros its accumulators start from.  false is the kernel as it was without the flag.
template <int DP, int AP, bool VCLIP, bool BC = false>
__global__ __launch_bounds__(256) void k_ppo_grad(GradArgs G, const float *__restrict__ weights, const long long *__restrict__ rows,
                                                  const float *__restrict__ obs, const uint8_t *__restrict__ mask,
                                                  const int *__restrict__ actions, const float *__restrict__ old_logp,
                                                  const float *__restrict__ adv, const float *__restrict__ ret,
                                                  const double *__restrict__ adv_partial, float *__restrict__ slabs,
                                                  const int *__restrict__ control, const float *__restrict__ old_values)
{
    // the body needs: DP, AP, VCLIP, BC (template parameters), KICK, K, SHARD, S and the arguments above
    constexpr bool KICK = false, SHARD = false;
    [[maybe_unused]] const KickArgs K{nullptr, 0.0f};
    [[maybe_unused]] const ShardArgs S{0, nullptr};
#include "mse_ppo_grad_body.inc"
}

// KICK: PPO with an imitation term (mse_ppo_bc_loss_grad).  The actor reads K.expert_actions at the row it reads `actions` at,
// its head is policy_bc_head_terms with K.bc_coef, and it carries seven sums (ce, hits, unusable rows after the four); the slab
// is slab_stride_kick wide and the misc strip kKickMiscFloats long.  The critic, the advantage pass, the gate, the row clamping
// and the grid rule are the same statements (mse_ppo_grad_body.inc).
template <int DP, int AP, bool VCLIP>
__global__ __launch_bounds__(256) void k_ppo_grad_kick(GradArgs G, const float *__restrict__ weights, const long long *__restrict__ rows,
                                                       const float *__restrict__ obs, const uint8_t *__restrict__ mask,
                                                       const int *__restrict__ actions, const float *__restrict__ old_logp,
                                                       const float *__restrict__ adv, const float *__restrict__ ret,
                                                       const double *__restrict__ adv_partial, float *__restrict__ slabs,
                                                       const int *__restrict__ control, const float *__restrict__ old_values,
                                                       KickArgs K)
{
    // the body needs: DP, AP, VCLIP (template parameters), BC, KICK, K, SHARD, S and the arguments above
    constexpr bool BC = false, KICK = true, SHARD = false;
    [[maybe_unused]] const ShardArgs S{0, nullptr};
#include "mse_ppo_grad_body.inc"
}

// SHARD: one shard of a minibatch whose rows live in several places (mse_ppo_shard_loss_grad).  G.batch is the number of LOCAL
// rows (the tile loop's bound and the row clamp are unchanged), every per-row term is scaled by 1 / S.global_batch, and the
// advantage mean and std come from S.moments, the sums over all shards (G.n_adv_partial is only the "normalise" flag;
// adv_partial is not an argument).  The slab is the other kernels'.  Everything else is the same statements.
template <int DP, int AP, bool VCLIP>
__global__ __launch_bounds__(256) void k_ppo_grad_shard(GradArgs G, const float *__restrict__ weights, const long long *__restrict__ rows,
                                                        const float *__restrict__ obs, const uint8_t *__restrict__ mask,
                                                        const int *__restrict__ actions, const float *__restrict__ old_logp,
                                                        const float *__restrict__ adv, const float *__restrict__ ret,
                                                        float *__restrict__ slabs, const int *__restrict__ control,
                                                        const float *__restrict__ old_values, ShardArgs S)
{
    // the body needs: DP, AP, VCLIP (template parameters), BC, KICK, K, SHARD, S and the arguments above
    constexpr bool BC = false, KICK = false, SHARD = true;
    [[maybe_unused]] const KickArgs K{nullptr, 0.0f};
    [[maybe_unused]] const double *adv_partial = nullptr; // named by the branch SHARD discards
#include "mse_ppo_grad_body.inc"
}

// grad_out[i] = sum over slabs, in slab order, in double; the last workgroup turns the loss sums into stats_out
// KICK: the slabs are slab_stride_kick apart; stats_out is f32[12]: [0] gains bc_coef * bc_loss, [8] bc_loss = mean ce,
// [9] hits / batch, [10] unusable rows / batch, [11] 0.  false is the kernel as it was without the flag and never reads bc_coef.
template <bool KICK>
__device__ __forceinline__ void ppo_reduce_body(const GradArgs &G, int n_slabs, int w_total, const float *__restrict__ slabs,
                                                const long long *__restrict__ rows, const float *__restrict__ adv,
                                                const double *__restrict__ adv_partial, float *__restrict__ grad_out,
                                                float *__restrict__ stats_out, const Gate &gate, float bc_coef)
{
    const long long stride = KICK ? slab_stride_kick(w_total) : slab_stride(w_total);
    if (gate.control != nullptr && slabs[w_total + kGateCell] != 0.0f) return; // the gate as k_ppo_grad saw it
    if (blockIdx.x + 1 < gridDim.x) {
        const int i = blockIdx.x * 256 + threadIdx.x;
        if (i >= w_total) return;
        double s = 0.0;
#pragma unroll 8
        for (int g = 0; g < n_slabs; ++g) s += (double)slabs[(long long)g * stride + i];
        grad_out[i] = (float)s;
        return;
    }
    __shared__ double sums[KICK ? kKickStatFloats : kStatFloats];
    if (threadIdx.x < kStatSums || (KICK && threadIdx.x >= kKickCe && threadIdx.x < kKickCe + 3)) {
        double s = 0.0;
#pragma unroll 8
        for (int g = 0; g < n_slabs; ++g) s += (double)slabs[(long long)g * stride + w_total + threadIdx.x];
        sums[threadIdx.x] = s / (double)G.batch;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float mean = 0.0f, std = 1.0f;
        if (G.n_adv_partial > 0) adv_mean_std(adv_partial, G.n_adv_partial, (double)adv[row_at(rows, 0, G.n_rows)], G.batch, mean, std);
        const double policy_loss = sums[0], value_loss = sums[1], entropy_loss = -sums[2];
        if constexpr (KICK) {
            const double bc_loss = sums[kKickCe];
            stats_out[0] = (float)(policy_loss + (double)G.P.ent_coef * entropy_loss + (double)G.P.vf_coef * value_loss + (double)bc_coef * bc_loss);
            stats_out[8] = (float)bc_loss;
            stats_out[9] = (float)sums[kKickCe + 1];
            stats_out[10] = (float)sums[kKickCe + 2];
            stats_out[11] = 0.0f;
        } else {
            stats_out[0] = (float)(policy_loss + (double)G.P.ent_coef * entropy_loss + (double)G.P.vf_coef * value_loss);
        }
        stats_out[1] = (float)policy_loss;
        stats_out[2] = (float)value_loss;
        stats_out[3] = (float)entropy_loss;
        stats_out[4] = (float)sums[3];
        stats_out[5] = (float)sums[4];
        stats_out[6] = mean;
        stats_out[7] = std;
        if (gate.control != nullptr) {
            gate.control[1] = gate.control[1] + 1;
            // SB3: `approx_kl_div > 1.5 * self.target_kl`, a float32 mean against a Python float
            if (gate.kl_limit > 0.0 && (double)stats_out[4] > gate.kl_limit) gate.control[0] = 1;
        }
    }
}

__global__ __launch_bounds__(256) void k_ppo_reduce(GradArgs G, int n_slabs, int w_total, const float *__restrict__ slabs,
                                                    const long long *__restrict__ rows, const float *__restrict__ adv,
                                                    const double *__restrict__ adv_partial, float *__restrict__ grad_out,
                                                    float *__restrict__ stats_out, Gate gate)
{
    ppo_reduce_body<false>(G, n_slabs, w_total, slabs, rows, adv, adv_partial, grad_out, stats_out, gate, 0.0f);
}

__global__ __launch_bounds__(256) void k_ppo_reduce_kick(GradArgs G, int n_slabs, int w_total, const float *__restrict__ slabs,
                                                         const long long *__restrict__ rows, const float *__restrict__ adv,
                                                         const double *__restrict__ adv_partial, float *__restrict__ grad_out,
                                                         float *__restrict__ stats_out, Gate gate, float bc_coef)
{
    ppo_reduce_body<true>(G, n_slabs, w_total, slabs, rows, adv, adv_partial, grad_out, stats_out, gate, bc_coef);
}

// ---- the three phases of a sharded minibatch (mse_ppo_shard_*) ---------------------------------------------------------------
// partial[2 g], partial[2 g + 1]: sum a and sum a^2 of workgroup g's rows, in double (no pivot: shards must add up)
__global__ __launch_bounds__(256) void k_ppo_shard_moments_partial(long long batch, long long n_rows, const long long *__restrict__ rows,
                                                                   const float *__restrict__ adv, double *__restrict__ partial,
                                                                   const int *__restrict__ control)
{
    __shared__ double sh[2][256];
    if (gate_closed(control)) return;
    double s = 0.0, q = 0.0;
    for (long long b = (long long)blockIdx.x * 256 + threadIdx.x; b < batch; b += (long long)gridDim.x * 256) {
        const double a = (double)adv[row_at(rows, b, n_rows)];
        s += a;
        q += a * a;
    }
    sh[0][threadIdx.x] = s;
    sh[1][threadIdx.x] = q;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) { // fixed tree
        if ((int)threadIdx.x < w) {
            sh[0][threadIdx.x] += sh[0][threadIdx.x + w];
            sh[1][threadIdx.x] += sh[1][threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = sh[0][0];
        partial[2 * blockIdx.x + 1] = sh[1][0];
    }
}

// one lane adds the partials in index order: moments_out = {count, sum a, sum a^2, 0}; n_partial = 0 (no local row) gives zeros
__global__ __launch_bounds__(64) void k_ppo_shard_moments_finish(long long batch, int n_partial, const double *__restrict__ partial,
                                                                 double *__restrict__ moments_out, const int *__restrict__ control)
{
    if (gate_closed(control) || threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0, q = 0.0;
    for (int g = 0; g < n_partial; ++g) {
        s += partial[2 * g];
        q += partial[2 * g + 1];
    }
    moments_out[0] = (double)batch;
    moments_out[1] = s;
    moments_out[2] = q;
    moments_out[3] = 0.0;
}

// partial_out[i] = sum over the slabs, in slab order, in double, for the W gradient cells and the kStatSums statistic cells
// behind them (which sit behind each other in a slab too); the padding cells are 0.  n_slabs = 0 (no local row) writes zeros.
// Nothing of this launch or the gradient launch before it writes the control block, so the gate is read as it stands.
__global__ __launch_bounds__(256) void k_ppo_shard_reduce(int n_slabs, int w_total, const float *__restrict__ slabs,
                                                          double *__restrict__ partial_out, const int *__restrict__ control)
{
    if (gate_closed(control)) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= (int)shard_partial_len(w_total)) return;
    const long long stride = slab_stride(w_total);
    double s = 0.0;
    if (i < w_total + kStatSums) {
#pragma unroll 8
        for (int g = 0; g < n_slabs; ++g) s += (double)slabs[(long long)g * stride + i];
    }
    partial_out[i] = s;
}

// ONE workgroup (a policy has at most 4 791 weights), so that every lane has read the gate before the one lane that may close
// it writes: grad_out[i] = (float)reduced[i]; lane 0 turns the statistic sums into stats_out exactly as k_ppo_reduce does,
// counts the minibatch and takes the target_kl decision.
__global__ __launch_bounds__(1024) void k_ppo_shard_finish(GradArgs G, int w_total, const double *__restrict__ reduced,
                                                           const double *__restrict__ moments, float *__restrict__ grad_out,
                                                           float *__restrict__ stats_out, Gate gate)
{
    const bool closed = gate_closed(gate.control);
    __syncthreads(); // every lane holds the gate as it was on entry
    if (closed) return;
    for (int i = threadIdx.x; i < w_total; i += 1024) grad_out[i] = (float)reduced[i];
    if (threadIdx.x == 0) {
        double sums[kStatSums];
#pragma unroll
        for (int k = 0; k < kStatSums; ++k) sums[k] = reduced[w_total + k] / (double)G.batch;
        float mean = 0.0f, std = 1.0f;
        if (G.n_adv_partial > 0) shard_mean_std(moments, G.batch, mean, std);
        const double policy_loss = sums[0], value_loss = sums[1], entropy_loss = -sums[2];
        stats_out[0] = (float)(policy_loss + (double)G.P.ent_coef * entropy_loss + (double)G.P.vf_coef * value_loss);
        stats_out[1] = (float)policy_loss;
        stats_out[2] = (float)value_loss;
        stats_out[3] = (float)entropy_loss;
        stats_out[4] = (float)sums[3];
        stats_out[5] = (float)sums[4];
        stats_out[6] = mean;
        stats_out[7] = std;
        if (gate.control != nullptr) {
            gate.control[1] = gate.control[1] + 1;
            if (gate.kl_limit > 0.0 && (double)stats_out[4] > gate.kl_limit) gate.control[0] = 1; // k_ppo_reduce's rule
        }
    }
}

// ---- clip_grad_norm_ + Adam, one workgroup ----------------------------------------------------------------------------
struct AdamArgs {
    int n;
    float lr_over_bc1, inv_sqrt_bc2, beta1, beta2, eps, max_norm;
    // 1 - beta, formed in double on the host and rounded once, as torch's addcmul_(value = 1 - beta2) does (the float32
    // difference 1.0f - 0.999f is 1.3e-5 below 0.001)
    float one_minus_beta1, one_minus_beta2;
};

__global__ __launch_bounds__(1024) void k_ppo_adam(AdamArgs a, float *__restrict__ w, const float *__restrict__ grad,
                                                   float *__restrict__ m, float *__restrict__ v, float *__restrict__ norm_out,
                                                   const int *__restrict__ control)
{
    __shared__ double sh[1024];
    if (gate_closed(control)) return;
    double s = 0.0;
    for (int i = threadIdx.x; i < a.n; i += 1024) s += (double)grad[i] * (double)grad[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int k = 512; k > 0; k >>= 1) { // fixed tree
        if ((int)threadIdx.x < k) sh[threadIdx.x] += sh[threadIdx.x + k];
        __syncthreads();
    }
    const float norm = (float)sqrt(sh[0]);
    float coef = 1.0f;
    if (a.max_norm > 0.0f) coef = fminf(1.0f, a.max_norm / (norm + 1e-6f));
    if (threadIdx.x == 0 && norm_out != nullptr) norm_out[0] = norm;
    for (int i = threadIdx.x; i < a.n; i += 1024) {
        const float g = grad[i] * coef;
        const float mi = a.beta1 * m[i] + a.one_minus_beta1 * g;
        const float vi = a.beta2 * v[i] + a.one_minus_beta2 * g * g;
        m[i] = mi;
        v[i] = vi;
        const float denom = sqrtf(vi) * a.inv_sqrt_bc2 + a.eps;
        w[i] = w[i] - a.lr_over_bc1 * (mi / denom);
    }
}

// ---- the minibatch shuffle: rows_out[j] = perm(first + j), j < count ----------------------------------------------------
// A lane takes two consecutive outputs per trip and stores them as one 16-byte word; `head` (0 or 1) outputs in front
// bring the pairs onto a 16-byte boundary (rows_out itself is only 8-byte aligned), and an odd one may be left at the
// end.  Lanes 0 and 1 of the grid write those two with 8-byte stores.
constexpr int kShuffleRowsPerGroup = 512; // 256 lanes x 2 rows per trip of the grid-stride loop
constexpr int kShuffleGroupsPerCu = 8;    // the grid cap: 32 waves per CU

__global__ __launch_bounds__(256) void k_ppo_shuffle(ShuffleKey key, uint32_t total, int bits, uint32_t first, long long count,
                                                     int head, long long *__restrict__ rows_out)
{
    const long long gtid = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long n_pairs = (count - head) >> 1;
    longlong2 *pairs = reinterpret_cast<longlong2 *>(rows_out + head);
    for (long long p = gtid; p < n_pairs; p += (long long)gridDim.x * 256) {
        const uint32_t i = first + (uint32_t)head + 2u * (uint32_t)p;
        longlong2 v;
        v.x = (long long)shuffle_index(key, total, bits, i);
        v.y = (long long)shuffle_index(key, total, bits, i + 1u);
        pairs[p] = v;
    }
    if (gtid == 0 && head != 0) rows_out[0] = (long long)shuffle_index(key, total, bits, first);
    const long long last = head + 2 * n_pairs;
    if (gtid == 1 && last < count) rows_out[last] = (long long)shuffle_index(key, total, bits, first + (uint32_t)last);
}

// the argument rules of both entry points; nullptr if they hold
const char *shuffle_args_error(int64_t total, int64_t first, int64_t count, const int64_t *rows_out)
{
    if (total < 1 || total > (int64_t)1 << 31) return "total must be in 1 .. 2^31";
    if (first < 0 || count < 0 || first > total || count > total - first) return "need 0 <= first, 0 <= count, first + count <= total";
    if (count > 0 && rows_out == nullptr) return "null output";
    return nullptr;
}

// enqueues k_ppo_grad; a failed launch shows in hipGetLastError after k_ppo_reduce's
template <int DP, int AP>
void launch_grad(const GradArgs &G, int n_slabs, hipStream_t s, const float *weights, const long long *rows, const float *obs,
                 const uint8_t *mask, const int *actions, const float *old_logp, const float *adv, const float *ret,
                 const double *adv_partial, float *slabs, const int *control, const float *old_values)
{
    const size_t lds = (size_t)(Padded<DP, AP>::total + 4 * kStageFloats + kMiscFloats) * sizeof(float);
    if (old_values != nullptr)
        hipLaunchKernelGGL((k_ppo_grad<DP, AP, true>), dim3((unsigned)n_slabs), dim3(256), lds, s, G, weights, rows, obs, mask, actions,
                           old_logp, adv, ret, adv_partial, slabs, control, old_values);
    else
        hipLaunchKernelGGL((k_ppo_grad<DP, AP, false>), dim3((unsigned)n_slabs), dim3(256), lds, s, G, weights, rows, obs, mask, actions,
                           old_logp, adv, ret, adv_partial, slabs, control, old_values);
}

// enqueues the KICK entry of the same body: one more misc strip size, two more arguments
template <int DP, int AP>
void launch_grad_kick(const GradArgs &G, int n_slabs, hipStream_t s, const float *weights, const long long *rows, const float *obs,
                      const uint8_t *mask, const int *actions, const float *old_logp, const float *adv, const float *ret,
                      const double *adv_partial, float *slabs, const int *control, const float *old_values, const KickArgs &K)
{
    const size_t lds = (size_t)(Padded<DP, AP>::total + 4 * kStageFloats + kKickMiscFloats) * sizeof(float);
    if (old_values != nullptr)
        hipLaunchKernelGGL((k_ppo_grad_kick<DP, AP, true>), dim3((unsigned)n_slabs), dim3(256), lds, s, G, weights, rows, obs, mask, actions,
                           old_logp, adv, ret, adv_partial, slabs, control, old_values, K);
    else
        hipLaunchKernelGGL((k_ppo_grad_kick<DP, AP, false>), dim3((unsigned)n_slabs), dim3(256), lds, s, G, weights, rows, obs, mask, actions,
                           old_logp, adv, ret, adv_partial, slabs, control, old_values, K);
}

// enqueues the SHARD entry of the same body: no adv_partial, one more argument
template <int DP, int AP>
void launch_grad_shard(const GradArgs &G, int n_slabs, hipStream_t s, const float *weights, const long long *rows, const float *obs,
                       const uint8_t *mask, const int *actions, const float *old_logp, const float *adv, const float *ret, float *slabs,
                       const int *control, const float *old_values, const ShardArgs &S)
{
    const size_t lds = (size_t)(Padded<DP, AP>::total + 4 * kStageFloats + kMiscFloats) * sizeof(float);
    if (old_values != nullptr)
        hipLaunchKernelGGL((k_ppo_grad_shard<DP, AP, true>), dim3((unsigned)n_slabs), dim3(256), lds, s, G, weights, rows, obs, mask,
                           actions, old_logp, adv, ret, slabs, control, old_values, S);
    else
        hipLaunchKernelGGL((k_ppo_grad_shard<DP, AP, false>), dim3((unsigned)n_slabs), dim3(256), lds, s, G, weights, rows, obs, mask,
                           actions, old_logp, adv, ret, slabs, control, old_values, S);
}

// enqueues the BC instantiation of k_ppo_grad: no old log-probabilities, advantages, gate or old values
template <int DP, int AP>
void launch_grad_bc(const GradArgs &G, int n_slabs, hipStream_t s, const float *weights, const long long *rows, const float *obs,
                    const uint8_t *mask, const int *actions, const float *ret, float *slabs)
{
    const size_t lds = (size_t)(Padded<DP, AP>::total + 4 * kStageFloats + kMiscFloats) * sizeof(float);
    hipLaunchKernelGGL((k_ppo_grad<DP, AP, false, true>), dim3((unsigned)n_slabs), dim3(256), lds, s, G, weights, rows, obs, mask, actions,
                       (const float *)nullptr, (const float *)nullptr, ret, (const double *)nullptr, slabs, (const int *)nullptr,
                       (const float *)nullptr);
}

// mse_ppo_loss_grad (control == NULL), mse_ppo_loss_grad_gated, mse_ppo_loss_grad_matrix (matrix: the gradient launch is
// k_ppo_grad_matrix of mse_ppo_matrix.hip; everything around it is the same) and mse_ppo_loss_grad_vclip (old_values != NULL:
// the gradient launch is the VCLIP instantiation with clip_range_vf, which the entry point has checked); `who` names the
// entry point in messages.  mse_ppo_bc_loss_grad (kick): the KICK gradient launch of either arithmetic on expert_actions with
// bc_coef, wider slabs, and k_ppo_reduce_kick
int loss_grad(const char *who, int obs_dim, int n_actions, const float *weights_dev, int64_t n_rows, const int64_t *rows_dev,
              int64_t batch, const float *obs, const uint8_t *mask, const int32_t *actions, const float *old_logp,
              const float *advantages, const float *returns, const mse_ppo_params *params, float *grad_out, float *stats_out,
              void *workspace, void *stream, Gate gate, int arithmetic = 0, const float *old_values = nullptr,
              double clip_range_vf = 0.0, bool kick = false, const int32_t *expert_actions = nullptr, double bc_coef = 0.0)
{
    auto fail = [who](int status, const char *why) { return mse_internal_fail(status, (std::string(who) + ": " + why).c_str()); };
    if (weights_dev == nullptr || obs == nullptr || actions == nullptr || old_logp == nullptr || advantages == nullptr ||
        returns == nullptr || params == nullptr || grad_out == nullptr || stats_out == nullptr || workspace == nullptr)
        return fail(MSE_ERR_INVALID_ARGUMENT, "null argument");
    if (obs_dim < 1 || obs_dim > 32 || n_actions < 1 || n_actions > 32)
        return fail(MSE_ERR_INVALID_ARGUMENT, "obs_dim and n_actions must be in 1..32");
    if (params->struct_size != sizeof(mse_ppo_params))
        return fail(MSE_ERR_INVALID_ARGUMENT, "mse_ppo_params.struct_size mismatch");
    if (n_rows < 1 || batch < 1 || (rows_dev == nullptr && batch > n_rows))
        return fail(MSE_ERR_INVALID_ARGUMENT, "need 1 <= batch (<= n_rows without rows_dev)");
    if (!(params->clip_range >= 0.0f) || !std::isfinite(params->ent_coef) || !std::isfinite(params->vf_coef))
        return fail(MSE_ERR_INVALID_ARGUMENT, "bad clip_range / ent_coef / vf_coef");
    if ((reinterpret_cast<uintptr_t>(workspace) & 15u) != 0)
        return fail(MSE_ERR_ALIGNMENT, "workspace must be 16-byte aligned");
    // what only mse_ppo_loss_grad_vclip can get wrong, after everything above: the arithmetic, then the clipping range
    if (arithmetic != 0 && arithmetic != 1) return fail(MSE_ERR_INVALID_ARGUMENT, "arithmetic must be 0 (fma) or 1 (matrix)");
    const float c_vf = old_values != nullptr ? (float)clip_range_vf : 0.0f; // without old_values clip_range_vf is not read
    if (old_values != nullptr && !(std::isfinite(clip_range_vf) && c_vf > 0.0f && std::isfinite(c_vf)))
        return fail(MSE_ERR_INVALID_ARGUMENT, "clip_range_vf must be finite and > 0 (as a float32) with old_values");
    // what only mse_ppo_bc_loss_grad can get wrong, after everything above: the labels, then the coefficient
    if (kick && expert_actions == nullptr) return fail(MSE_ERR_INVALID_ARGUMENT, "null expert_actions");
    if (kick && !(std::isfinite(bc_coef) && bc_coef >= 0.0 && std::isfinite((float)bc_coef)))
        return fail(MSE_ERR_INVALID_ARGUMENT, "bc_coef must be finite and >= 0 (as a float32)");
    const KickArgs K{expert_actions, (float)bc_coef};
    const int cus = cu_count();
    if (cus <= 0) return fail(MSE_ERR_NO_DEVICE, "no HIP device (there is no CPU path)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    double *adv_partial = static_cast<double *>(workspace);
    float *slabs = reinterpret_cast<float *>(adv_partial + 2 * kMaxAdvPartials);
    const long long *rows = reinterpret_cast<const long long *>(rows_dev);
    GradArgs G{obs_dim, n_actions, (long long)n_rows, (long long)batch, 0,
               Params{params->clip_range, params->ent_coef, params->vf_coef, params->normalize_advantage, c_vf}};
    if (params->normalize_advantage != 0 && batch > 1) {
        long long g1 = (batch + 1023) / 1024;
        G.n_adv_partial = (int)(g1 > kMaxAdvPartials ? kMaxAdvPartials : g1);
        hipLaunchKernelGGL(k_ppo_adv_partial, dim3((unsigned)G.n_adv_partial), dim3(256), 0, s, (long long)batch, (long long)n_rows, rows,
                           advantages, adv_partial, gate.control);
    }
    const int n_slabs = (int)grad_groups(batch, cus);
    hipError_t e = hipSuccess;
    if (kick && arithmetic == 1) {
        e = mse_ppo_launch_grad_matrix_kick(G, n_slabs, s, weights_dev, rows, obs, mask, actions, old_logp, advantages, returns,
                                            adv_partial, slabs, gate.control, old_values, K);
    } else if (kick) {
#define MSE_PPO_LAUNCH_KICK(DP, AP)                                                                                                     \
    launch_grad_kick<DP, AP>(G, n_slabs, s, weights_dev, rows, obs, mask, actions, old_logp, advantages, returns, adv_partial, slabs, \
                             gate.control, old_values, K)
        MSE_PPO_DISPATCH(select_grad_shape(obs_dim, n_actions), MSE_PPO_LAUNCH_KICK);
#undef MSE_PPO_LAUNCH_KICK
    } else if (arithmetic == 1) {
        e = mse_ppo_launch_grad_matrix(G, n_slabs, s, weights_dev, rows, obs, mask, actions, old_logp, advantages, returns, adv_partial,
                                       slabs, gate.control, old_values);
    } else {
        // four shapes, chosen in mse_ppo_math.h: Env_1 (13 -> 2), Env_2 (16 -> 11), Env_3 (29 -> 22) and the general one
#define MSE_PPO_LAUNCH(DP, AP)                                                                                                     \
    launch_grad<DP, AP>(G, n_slabs, s, weights_dev, rows, obs, mask, actions, old_logp, advantages, returns, adv_partial, slabs, \
                        gate.control, old_values)
        MSE_PPO_DISPATCH(select_grad_shape(obs_dim, n_actions), MSE_PPO_LAUNCH);
#undef MSE_PPO_LAUNCH
    }
    if (e == hipSuccess) {
        const int w_total = flat_layout(obs_dim, n_actions).total;
        const dim3 grid((unsigned)((w_total + 255) / 256 + 1));
        if (kick)
            hipLaunchKernelGGL(k_ppo_reduce_kick, grid, dim3(256), 0, s, G, n_slabs, w_total, slabs, rows, advantages, adv_partial, grad_out,
                               stats_out, gate, K.bc_coef);
        else
            hipLaunchKernelGGL(k_ppo_reduce, grid, dim3(256), 0, s, G, n_slabs, w_total, slabs, rows, advantages, adv_partial, grad_out,
                               stats_out, gate);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return fail(MSE_ERR_HIP, "kernel launch failed");
    return MSE_OK;
}

int adam_step(const char *who, int64_t n_weights, float *weights, const float *grad, float *m, float *v, int64_t step, double lr,
              double beta1, double beta2, double eps, double max_grad_norm, float *grad_norm_out, void *stream, const int *control)
{
    auto fail = [who](int status, const char *why) { return mse_internal_fail(status, (std::string(who) + ": " + why).c_str()); };
    if (weights == nullptr || grad == nullptr || m == nullptr || v == nullptr) return fail(MSE_ERR_INVALID_ARGUMENT, "null argument");
    if (n_weights < 1 || n_weights > (1 << 24) || step < 1)
        return fail(MSE_ERR_INVALID_ARGUMENT, "need 1 <= n_weights <= 2^24 and step >= 1");
    if (!(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0))
        return fail(MSE_ERR_INVALID_ARGUMENT, "bad lr / beta / eps");
    const double bc1 = 1.0 - std::pow(beta1, (double)step), bc2 = 1.0 - std::pow(beta2, (double)step);
    AdamArgs a{(int)n_weights, (float)(lr / bc1), (float)(1.0 / std::sqrt(bc2)), (float)beta1, (float)beta2, (float)eps,
               (float)max_grad_norm, (float)(1.0 - beta1), (float)(1.0 - beta2)};
    hipLaunchKernelGGL(k_ppo_adam, dim3(1), dim3(1024), 0, static_cast<hipStream_t>(stream), a, weights, grad, m, v, grad_norm_out, control);
    if (hipGetLastError() != hipSuccess) return fail(MSE_ERR_HIP, "kernel launch failed");
    return MSE_OK;
}

} // namespace

extern "C" {

int mse_gae(int32_t k_steps, int64_t n, const float *rewards, const float *values, const uint8_t *episode_starts,
            const float *last_values, const uint8_t *last_dones, double gamma, double gae_lambda, float *advantages_out,
            float *returns_out, void *stream)
{
    if (rewards == nullptr || values == nullptr || episode_starts == nullptr || last_values == nullptr || last_dones == nullptr ||
        advantages_out == nullptr || returns_out == nullptr)
        return mse_internal_fail(MSE_ERR_INVALID_ARGUMENT, "mse_gae: null argument");
    if (k_steps < 1 || n < 1) return mse_internal_fail(MSE_ERR_INVALID_ARGUMENT, "mse_gae: k_steps and n must be positive");
    if (!(gamma >= 0.0 && gamma <= 1.0) || !(gae_lambda >= 0.0 && gae_lambda <= 1.0))
        return mse_internal_fail(MSE_ERR_INVALID_ARGUMENT, "mse_gae: gamma and gae_lambda must lie in [0, 1]");
    const long long blocks = (n + 255) / 256;
    hipLaunchKernelGGL(k_gae, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), (int)k_steps, (long long)n,
                       rewards, values, episode_starts, last_values, last_dones, (float)gamma, (float)(gamma * gae_lambda),
                       advantages_out, returns_out);
    if (hipGetLastError() != hipSuccess) return mse_internal_fail(MSE_ERR_HIP, "mse_gae: kernel launch failed");
    return MSE_OK;
}

int64_t mse_ppo_workspace_bytes(int obs_dim, int n_actions)
{
    if (obs_dim < 1 || obs_dim > 32 || n_actions < 1 || n_actions > 32) return 0;
    const long long w = flat_layout(obs_dim, n_actions).total;
    return (int64_t)(kMaxAdvPartials * 2 * sizeof(double) + (size_t)kMaxSlabs * slab_stride(w) * sizeof(float));
}

int mse_ppo_loss_grad(int obs_dim, int n_actions, const float *weights_dev, int64_t n_rows, const int64_t *rows_dev, int64_t batch,
                      const float *obs, const uint8_t *mask, const int32_t *actions, const float *old_logp,
                      const float *advantages, const float *returns, const mse_ppo_params *params, float *grad_out,
                      float *stats_out, void *workspace, void *stream)
{
    return loss_grad("mse_ppo_loss_grad", obs_dim, n_actions, weights_dev, n_rows, rows_dev, batch, obs, mask, actions, old_logp,
                     advantages, returns, params, grad_out, stats_out, workspace, stream, Gate{nullptr, 0.0});
}

int mse_ppo_loss_grad_gated(int obs_dim, int n_actions, const float *weights_dev, int64_t n_rows, const int64_t *rows_dev,
                            int64_t batch, const float *obs, const uint8_t *mask, const int32_t *actions, const float *old_logp,
                            const float *advantages, const float *returns, const mse_ppo_params *params, float *grad_out,
                            float *stats_out, void *workspace, void *stream, double target_kl, int32_t *control_dev)
{
    if (control_dev == nullptr) return mse_internal_fail(MSE_ERR_INVALID_ARGUMENT, "mse_ppo_loss_grad_gated: null control block");
    if (target_kl != target_kl) return mse_internal_fail(MSE_ERR_INVALID_ARGUMENT, "mse_ppo_loss_grad_gated: target_kl is NaN");
    return loss_grad("mse_ppo_loss_grad_gated", obs_dim, n_actions, weights_dev, n_rows, rows_dev, batch, obs, mask, actions, old_logp,
                     advantages, returns, params, grad_out, stats_out, workspace, stream, Gate{control_dev, 1.5 * target_kl});
}

int mse_ppo_loss_grad_matrix(int obs_dim, int n_actions, const float *weights_dev, int64_t n_rows, const int64_t *rows_dev,
                             int64_t batch, const float *obs, const uint8_t *mask, const int32_t *actions, const float *old_logp,
                             const float *advantages, const float *returns, const mse_ppo_params *params, float *grad_out,
                             float *stats_out, void *workspace, void *stream, double target_kl, int32_t *control_dev)
{
    if (control_dev != nullptr && target_kl != target_kl)
        return mse_internal_fail(MSE_ERR_INVALID_ARGUMENT, "mse_ppo_loss_grad_matrix: target_kl is NaN");
    return loss_grad("mse_ppo_loss_grad_matrix", obs_dim, n_actions, weights_dev, n_rows, rows_dev, batch, obs, mask, actions, old_logp,
                     advantages, returns, params, grad_out, stats_out, workspace, stream,
                     control_dev == nullptr ? Gate{nullptr, 0.0} : Gate{control_dev, 1.5 * target_kl}, 1);
}

int mse_ppo_loss_grad_vclip(int obs_dim, int n_actions, const float *weights_dev, int64_t n_rows, const int64_t *rows_dev,
                            int64_t batch, const float *obs, const uint8_t *mask, const int32_t *actions, const float *old_logp,
                            const float *advantages, const float *returns, const mse_ppo_params *params, float *grad_out,
                            float *stats_out, void *workspace, void *stream, double target_kl, int32_t *control_dev, int arithmetic,
                            const float *old_values, double clip_range_vf)
{
    if (control_dev != nullptr && target_kl != target_kl)
        return mse_internal_fail(MSE_ERR_INVALID_ARGUMENT, "mse_ppo_loss_grad_vclip: target_kl is NaN");
    return loss_grad("mse_ppo_loss_grad_vclip", obs_dim, n_actions, weights_dev, n_rows, rows_dev, batch, obs, mask, actions, old_logp,
                     advantages, returns, params, grad_out, stats_out, workspace, stream,
                     control_dev == nullptr ? Gate{nullptr, 0.0} : Gate{control_dev, 1.5 * target_kl}, arithmetic, old_values,
                     clip_range_vf);
}

// ---- mse_ppo_loss_grad_vclip for a minibatch whose rows live in several places: moments, partial, finish -----------------------
int64_t mse_ppo_shard_partial_len(int obs_dim, int n_actions)
{
    if (obs_dim < 1 || obs_dim > 32 || n_actions < 1 || n_actions > 32) return 0;
    return (int64_t)shard_partial_len(flat_layout(obs_dim, n_actions).total);
}

int mse_ppo_shard_moments(int64_t n_rows, const int64_t *rows_dev, int64_t batch_local, const float *advantages, double *moments_out,
                          void *workspace, void *stream, const int32_t *control_dev)
{
    auto fail = [](int status, const char *why) { return mse_internal_fail(status, (std::string("mse_ppo_shard_moments: ") + why).c_str()); };
    if (advantages == nullptr || moments_out == nullptr || workspace == nullptr) return fail(MSE_ERR_INVALID_ARGUMENT, "null argument");
    if (n_rows < 1 || batch_local < 0 || (rows_dev == nullptr && batch_local > n_rows))
        return fail(MSE_ERR_INVALID_ARGUMENT, "need 0 <= batch_local (<= n_rows without rows_dev)");
    if ((reinterpret_cast<uintptr_t>(workspace) & 15u) != 0) return fail(MSE_ERR_ALIGNMENT, "workspace must be 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(moments_out) & 7u) != 0) return fail(MSE_ERR_ALIGNMENT, "moments_out must be 8-byte aligned");
    if (cu_count() <= 0) return fail(MSE_ERR_NO_DEVICE, "no HIP device (there is no CPU path)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    double *partial = static_cast<double *>(workspace);
    int n_partial = 0;
    if (batch_local > 0) {
        const long long g1 = (batch_local + 1023) / 1024;
        n_partial = (int)(g1 > kMaxAdvPartials ? kMaxAdvPartials : g1);
        hipLaunchKernelGGL(k_ppo_shard_moments_partial, dim3((unsigned)n_partial), dim3(256), 0, s, (long long)batch_local, (long long)n_rows,
                           reinterpret_cast<const long long *>(rows_dev), advantages, partial, control_dev);
    }
    hipLaunchKernelGGL(k_ppo_shard_moments_finish, dim3(1), dim3(64), 0, s, (long long)batch_local, n_partial, partial, moments_out,
                       control_dev);
    if (hipGetLastError() != hipSuccess) return fail(MSE_ERR_HIP, "kernel launch failed");
    return MSE_OK;
}

int mse_ppo_shard_loss_grad(int obs_dim, int n_actions, const float *weights_dev, int64_t n_rows, const int64_t *rows_dev,
                            int64_t batch_local, const float *obs, const uint8_t *mask, const int32_t *actions, const float *old_logp,
                            const float *advantages, const float *returns, const mse_ppo_params *params, int64_t global_batch,
                            const double *moments_dev, double *partial_out, void *workspace, void *stream, const int32_t *control_dev,
                            int arithmetic, const float *old_values, double clip_range_vf)
{
    auto fail = [](int status, const char *why) { return mse_internal_fail(status, (std::string("mse_ppo_shard_loss_grad: ") + why).c_str()); };
    if (weights_dev == nullptr || obs == nullptr || actions == nullptr || old_logp == nullptr || advantages == nullptr ||
        returns == nullptr || params == nullptr || moments_dev == nullptr || partial_out == nullptr || workspace == nullptr)
        return fail(MSE_ERR_INVALID_ARGUMENT, "null argument");
    if (obs_dim < 1 || obs_dim > 32 || n_actions < 1 || n_actions > 32)
        return fail(MSE_ERR_INVALID_ARGUMENT, "obs_dim and n_actions must be in 1..32");
    if (params->struct_size != sizeof(mse_ppo_params)) return fail(MSE_ERR_INVALID_ARGUMENT, "mse_ppo_params.struct_size mismatch");
    if (n_rows < 1 || batch_local < 0 || (rows_dev == nullptr && batch_local > n_rows))
        return fail(MSE_ERR_INVALID_ARGUMENT, "need 0 <= batch_local (<= n_rows without rows_dev)");
    if (global_batch < 1 || global_batch < batch_local)
        return fail(MSE_ERR_INVALID_ARGUMENT, "need global_batch >= max(1, batch_local)");
    if (!(params->clip_range >= 0.0f) || !std::isfinite(params->ent_coef) || !std::isfinite(params->vf_coef))
        return fail(MSE_ERR_INVALID_ARGUMENT, "bad clip_range / ent_coef / vf_coef");
    if ((reinterpret_cast<uintptr_t>(workspace) & 15u) != 0) return fail(MSE_ERR_ALIGNMENT, "workspace must be 16-byte aligned");
    if (((reinterpret_cast<uintptr_t>(moments_dev) | reinterpret_cast<uintptr_t>(partial_out)) & 7u) != 0)
        return fail(MSE_ERR_ALIGNMENT, "moments_dev and partial_out must be 8-byte aligned");
    if (arithmetic != 0 && arithmetic != 1) return fail(MSE_ERR_INVALID_ARGUMENT, "arithmetic must be 0 (fma) or 1 (matrix)");
    const float c_vf = old_values != nullptr ? (float)clip_range_vf : 0.0f; // without old_values clip_range_vf is not read
    if (old_values != nullptr && !(std::isfinite(clip_range_vf) && c_vf > 0.0f && std::isfinite(c_vf)))
        return fail(MSE_ERR_INVALID_ARGUMENT, "clip_range_vf must be finite and > 0 (as a float32) with old_values");
    const int cus = cu_count();
    if (cus <= 0) return fail(MSE_ERR_NO_DEVICE, "no HIP device (there is no CPU path)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    float *slabs = reinterpret_cast<float *>(static_cast<double *>(workspace) + 2 * kMaxAdvPartials); // mse_ppo_loss_grad's layout
    const long long *rows = reinterpret_cast<const long long *>(rows_dev);
    // G.batch bounds the local rows; n_adv_partial is the "normalise" flag: the existing rule applied to the global count
    const GradArgs G{obs_dim, n_actions, (long long)n_rows, (long long)batch_local,
                     params->normalize_advantage != 0 && global_batch > 1 ? 1 : 0,
                     Params{params->clip_range, params->ent_coef, params->vf_coef, params->normalize_advantage, c_vf}};
    const ShardArgs S{(long long)global_batch, moments_dev};
    const int n_slabs = batch_local > 0 ? (int)grad_groups(batch_local, cus) : 0;
    hipError_t e = hipSuccess;
    if (n_slabs == 0) {
        // no local row: no gradient launch, the reduction below writes zeros
    } else if (arithmetic == 1) {
        e = mse_ppo_launch_grad_matrix_shard(G, n_slabs, s, weights_dev, rows, obs, mask, actions, old_logp, advantages, returns, slabs,
                                             control_dev, old_values, S);
    } else {
#define MSE_PPO_LAUNCH_SHARD(DP, AP)                                                                                                  \
    launch_grad_shard<DP, AP>(G, n_slabs, s, weights_dev, rows, obs, mask, actions, old_logp, advantages, returns, slabs, control_dev, \
                              old_values, S)
        MSE_PPO_DISPATCH(select_grad_shape(obs_dim, n_actions), MSE_PPO_LAUNCH_SHARD);
#undef MSE_PPO_LAUNCH_SHARD
    }
    if (e == hipSuccess) {
        const int w_total = flat_layout(obs_dim, n_actions).total;
        const int len = (int)shard_partial_len(w_total);
        hipLaunchKernelGGL(k_ppo_shard_reduce, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, s, n_slabs, w_total, slabs, partial_out,
                           control_dev);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return fail(MSE_ERR_HIP, "kernel launch failed");
    return MSE_OK;
}

int mse_ppo_shard_finish(int obs_dim, int n_actions, int64_t global_batch, const double *reduced_dev, const double *moments_dev,
                         const mse_ppo_params *params, float *grad_out, float *stats_out, void *stream, double target_kl,
                         int32_t *control_dev)
{
    auto fail = [](int status, const char *why) { return mse_internal_fail(status, (std::string("mse_ppo_shard_finish: ") + why).c_str()); };
    if (control_dev != nullptr && target_kl != target_kl) return fail(MSE_ERR_INVALID_ARGUMENT, "target_kl is NaN");
    if (reduced_dev == nullptr || moments_dev == nullptr || params == nullptr || grad_out == nullptr || stats_out == nullptr)
        return fail(MSE_ERR_INVALID_ARGUMENT, "null argument");
    if (obs_dim < 1 || obs_dim > 32 || n_actions < 1 || n_actions > 32)
        return fail(MSE_ERR_INVALID_ARGUMENT, "obs_dim and n_actions must be in 1..32");
    if (params->struct_size != sizeof(mse_ppo_params)) return fail(MSE_ERR_INVALID_ARGUMENT, "mse_ppo_params.struct_size mismatch");
    if (global_batch < 1) return fail(MSE_ERR_INVALID_ARGUMENT, "need global_batch >= 1");
    if (!std::isfinite(params->ent_coef) || !std::isfinite(params->vf_coef)) return fail(MSE_ERR_INVALID_ARGUMENT, "bad ent_coef / vf_coef");
    if (((reinterpret_cast<uintptr_t>(reduced_dev) | reinterpret_cast<uintptr_t>(moments_dev)) & 7u) != 0)
        return fail(MSE_ERR_ALIGNMENT, "reduced_dev and moments_dev must be 8-byte aligned");
    if (cu_count() <= 0) return fail(MSE_ERR_NO_DEVICE, "no HIP device (there is no CPU path)");
    // batch = the global count (the divisor of the statistic sums); n_adv_partial = the "normalise" flag, mse_ppo_shard_loss_grad's
    const GradArgs G{obs_dim, n_actions, 0, (long long)global_batch, params->normalize_advantage != 0 && global_batch > 1 ? 1 : 0,
                     Params{params->clip_range, params->ent_coef, params->vf_coef, params->normalize_advantage, 0.0f}};
    const Gate gate = control_dev == nullptr ? Gate{nullptr, 0.0} : Gate{control_dev, 1.5 * target_kl};
    hipLaunchKernelGGL(k_ppo_shard_finish, dim3(1), dim3(1024), 0, static_cast<hipStream_t>(stream), G,
                       flat_layout(obs_dim, n_actions).total, reduced_dev, moments_dev, grad_out, stats_out, gate);
    if (hipGetLastError() != hipSuccess) return fail(MSE_ERR_HIP, "kernel launch failed");
    return MSE_OK;
}

int64_t mse_ppo_bc_workspace_bytes(int obs_dim, int n_actions)
{
    if (obs_dim < 1 || obs_dim > 32 || n_actions < 1 || n_actions > 32) return 0;
    const long long w = flat_layout(obs_dim, n_actions).total;
    return (int64_t)(kMaxAdvPartials * 2 * sizeof(double) + (size_t)kMaxSlabs * slab_stride_kick(w) * sizeof(float));
}

int mse_ppo_bc_loss_grad(int obs_dim, int n_actions, const float *weights_dev, int64_t n_rows, const int64_t *rows_dev, int64_t batch,
                         const float *obs, const uint8_t *mask, const int32_t *actions, const float *old_logp,
                         const float *advantages, const float *returns, const mse_ppo_params *params, float *grad_out,
                         float *stats_out, void *workspace, void *stream, double target_kl, int32_t *control_dev, int arithmetic,
                         const float *old_values, double clip_range_vf, const int32_t *expert_actions, double bc_coef)
{
    if (control_dev != nullptr && target_kl != target_kl)
        return mse_internal_fail(MSE_ERR_INVALID_ARGUMENT, "mse_ppo_bc_loss_grad: target_kl is NaN");
    return loss_grad("mse_ppo_bc_loss_grad", obs_dim, n_actions, weights_dev, n_rows, rows_dev, batch, obs, mask, actions, old_logp,
                     advantages, returns, params, grad_out, stats_out, workspace, stream,
                     control_dev == nullptr ? Gate{nullptr, 0.0} : Gate{control_dev, 1.5 * target_kl}, arithmetic, old_values,
                     clip_range_vf, true, expert_actions, bc_coef);
}

int mse_bc_loss_grad(int obs_dim, int n_actions, const float *weights_dev, int64_t n_rows, const int64_t *rows_dev, int64_t batch,
                     const float *obs, const uint8_t *mask, const int32_t *actions, const float *returns,
                     const mse_ppo_params *params, float *grad_out, float *stats_out, void *workspace, void *stream, int arithmetic)
{
    auto fail = [](int status, const char *why) { return mse_internal_fail(status, (std::string("mse_bc_loss_grad: ") + why).c_str()); };
    if (weights_dev == nullptr || obs == nullptr || actions == nullptr || params == nullptr || grad_out == nullptr ||
        stats_out == nullptr || workspace == nullptr)
        return fail(MSE_ERR_INVALID_ARGUMENT, "null argument");
    if (obs_dim < 1 || obs_dim > 32 || n_actions < 1 || n_actions > 32)
        return fail(MSE_ERR_INVALID_ARGUMENT, "obs_dim and n_actions must be in 1..32");
    if (params->struct_size != sizeof(mse_ppo_params))
        return fail(MSE_ERR_INVALID_ARGUMENT, "mse_ppo_params.struct_size mismatch");
    if (n_rows < 1 || batch < 1 || (rows_dev == nullptr && batch > n_rows))
        return fail(MSE_ERR_INVALID_ARGUMENT, "need 1 <= batch (<= n_rows without rows_dev)");
    if (!std::isfinite(params->ent_coef) || !std::isfinite(params->vf_coef))
        return fail(MSE_ERR_INVALID_ARGUMENT, "bad ent_coef / vf_coef");
    if ((reinterpret_cast<uintptr_t>(workspace) & 15u) != 0)
        return fail(MSE_ERR_ALIGNMENT, "workspace must be 16-byte aligned");
    if (arithmetic != 0 && arithmetic != 1) return fail(MSE_ERR_INVALID_ARGUMENT, "arithmetic must be 0 (fma) or 1 (matrix)");
    const int cus = cu_count();
    if (cus <= 0) return fail(MSE_ERR_NO_DEVICE, "no HIP device (there is no CPU path)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    double *adv_partial = static_cast<double *>(workspace); // the workspace's layout is mse_ppo_loss_grad's; these are not used
    float *slabs = reinterpret_cast<float *>(adv_partial + 2 * kMaxAdvPartials);
    const long long *rows = reinterpret_cast<const long long *>(rows_dev);
    // clip_range and normalize_advantage are not read; n_adv_partial = 0: k_ppo_reduce writes stats_out[6..7] = 0, 1
    const GradArgs G{obs_dim, n_actions, (long long)n_rows, (long long)batch, 0, Params{0.0f, params->ent_coef, params->vf_coef, 0, 0.0f}};
    const int n_slabs = (int)grad_groups(batch, cus);
    hipError_t e = hipSuccess;
    if (arithmetic == 1) {
        e = mse_ppo_launch_grad_matrix_bc(G, n_slabs, s, weights_dev, rows, obs, mask, actions, returns, slabs);
    } else {
#define MSE_BC_LAUNCH(DP, AP) launch_grad_bc<DP, AP>(G, n_slabs, s, weights_dev, rows, obs, mask, actions, returns, slabs)
        MSE_PPO_DISPATCH(select_grad_shape(obs_dim, n_actions), MSE_BC_LAUNCH);
#undef MSE_BC_LAUNCH
    }
    if (e == hipSuccess) {
        const int w_total = flat_layout(obs_dim, n_actions).total;
        hipLaunchKernelGGL(k_ppo_reduce, dim3((unsigned)((w_total + 255) / 256 + 1)), dim3(256), 0, s, G, n_slabs, w_total, slabs, rows,
                           (const float *)nullptr, adv_partial, grad_out, stats_out, Gate{nullptr, 0.0});
        e = hipGetLastError();
    }
    if (e != hipSuccess) return fail(MSE_ERR_HIP, "kernel launch failed");
    return MSE_OK;
}

int64_t mse_explained_variance_workspace_bytes(void) { return (int64_t)(kEvMaxGroups * 4 * sizeof(double)); }

int mse_explained_variance(int64_t n, const float *values, const float *returns, float *out_dev, void *workspace, void *stream)
{
    if (const char *why = explained_variance_args_error(n, values, returns, out_dev))
        return mse_internal_fail(MSE_ERR_INVALID_ARGUMENT, (std::string("mse_explained_variance: ") + why).c_str());
    if (workspace == nullptr) return mse_internal_fail(MSE_ERR_INVALID_ARGUMENT, "mse_explained_variance: null workspace");
    if ((reinterpret_cast<uintptr_t>(workspace) & 7u) != 0)
        return mse_internal_fail(MSE_ERR_ALIGNMENT, "mse_explained_variance: workspace must be 8-byte aligned");
    if (cu_count() <= 0)
        return mse_internal_fail(MSE_ERR_NO_DEVICE, "mse_explained_variance: no HIP device (mse_explained_variance_host runs on the CPU)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    double *partial = static_cast<double *>(workspace);
    const int groups = ev_groups((long long)n);
    hipLaunchKernelGGL(k_explained_variance_partial, dim3((unsigned)groups), dim3(kEvLanes), 0, s, (long long)n, values, returns, partial);
    hipLaunchKernelGGL(k_explained_variance_finish, dim3(1), dim3(64), 0, s, (long long)n, groups, partial, out_dev);
    if (hipGetLastError() != hipSuccess) return mse_internal_fail(MSE_ERR_HIP, "mse_explained_variance: kernel launch failed");
    return MSE_OK;
}

int mse_explained_variance_host(int64_t n, const float *values, const float *returns, float *out)
{
    if (const char *why = explained_variance_args_error(n, values, returns, out))
        return mse_internal_fail(MSE_ERR_INVALID_ARGUMENT, (std::string("mse_explained_variance_host: ") + why).c_str());
    const int groups = ev_groups((long long)n);
    double sums[4] = {0.0, 0.0, 0.0, 0.0};
    std::vector<double> lanes(4 * kEvLanes);
    for (int g = 0; g < groups; ++g) { // the kernel's order: a lane's elements, the tree over the lanes, the groups in index order
        for (int t = 0; t < kEvLanes; ++t) {
            double acc[4] = {0.0, 0.0, 0.0, 0.0};
            ev_lane_sums((long long)n, (long long)g * kEvLanes + t, (long long)groups * kEvLanes, values, returns, acc);
            for (int k = 0; k < 4; ++k) lanes[k * kEvLanes + t] = acc[k];
        }
        for (int w = kEvLanes / 2; w > 0; w >>= 1)
            for (int t = 0; t < w; ++t)
                for (int k = 0; k < 4; ++k) lanes[k * kEvLanes + t] += lanes[k * kEvLanes + t + w];
        for (int k = 0; k < 4; ++k) sums[k] += lanes[k * kEvLanes];
    }
    out[0] = (float)ev_from_sums(sums, (long long)n);
    return MSE_OK;
}

int mse_ppo_adam_step(int64_t n_weights, float *weights, const float *grad, float *m, float *v, int64_t step, double lr,
                      double beta1, double beta2, double eps, double max_grad_norm, float *grad_norm_out, void *stream)
{
    return adam_step("mse_ppo_adam_step", n_weights, weights, grad, m, v, step, lr, beta1, beta2, eps, max_grad_norm, grad_norm_out,
                     stream, nullptr);
}

int mse_ppo_adam_step_gated(int64_t n_weights, float *weights, const float *grad, float *m, float *v, int64_t step, double lr,
                            double beta1, double beta2, double eps, double max_grad_norm, float *grad_norm_out, void *stream,
                            const int32_t *control_dev)
{
    if (control_dev == nullptr) return mse_internal_fail(MSE_ERR_INVALID_ARGUMENT, "mse_ppo_adam_step_gated: null control block");
    return adam_step("mse_ppo_adam_step_gated", n_weights, weights, grad, m, v, step, lr, beta1, beta2, eps, max_grad_norm,
                     grad_norm_out, stream, control_dev);
}

int mse_ppo_shuffle(int64_t total, uint64_t seed, uint64_t epoch, int64_t first, int64_t count, int64_t *rows_out_dev, void *stream)
{
    if (const char *why = shuffle_args_error(total, first, count, rows_out_dev))
        return mse_internal_fail(MSE_ERR_INVALID_ARGUMENT, (std::string("mse_ppo_shuffle: ") + why).c_str());
    if (count == 0) return MSE_OK;
    if ((reinterpret_cast<uintptr_t>(rows_out_dev) & 7u) != 0)
        return mse_internal_fail(MSE_ERR_ALIGNMENT, "mse_ppo_shuffle: rows_out_dev must be 8-byte aligned");
    const int cus = cu_count();
    if (cus <= 0) return mse_internal_fail(MSE_ERR_NO_DEVICE, "mse_ppo_shuffle: no HIP device (mse_ppo_shuffle_host runs on the CPU)");
    const int head = (int)((reinterpret_cast<uintptr_t>(rows_out_dev) >> 3) & 1u);
    long long groups = (count + kShuffleRowsPerGroup - 1) / kShuffleRowsPerGroup;
    const long long cap = (long long)kShuffleGroupsPerCu * cus;
    if (groups > cap) groups = cap;
    hipLaunchKernelGGL(k_ppo_shuffle, dim3((unsigned)groups), dim3(256), 0, static_cast<hipStream_t>(stream), shuffle_key(seed, epoch),
                       (uint32_t)total, shuffle_bits((uint32_t)total), (uint32_t)first, (long long)count, head,
                       reinterpret_cast<long long *>(rows_out_dev));
    if (hipGetLastError() != hipSuccess) return mse_internal_fail(MSE_ERR_HIP, "mse_ppo_shuffle: kernel launch failed");
    return MSE_OK;
}

int mse_ppo_shuffle_host(int64_t total, uint64_t seed, uint64_t epoch, int64_t first, int64_t count, int64_t *rows_out)
{
    if (const char *why = shuffle_args_error(total, first, count, rows_out))
        return mse_internal_fail(MSE_ERR_INVALID_ARGUMENT, (std::string("mse_ppo_shuffle_host: ") + why).c_str());
    const ShuffleKey key = shuffle_key(seed, epoch);
    const int bits = shuffle_bits((uint32_t)total);
    for (int64_t j = 0; j < count; ++j) rows_out[j] = (int64_t)shuffle_index(key, (uint32_t)total, bits, (uint32_t)(first + j));
    return MSE_OK;
}

} // extern "C"
