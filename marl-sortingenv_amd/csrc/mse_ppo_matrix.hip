// The PPO gradient of one minibatch on the f32 matrix cores (k_ppo_grad_matrix): what k_ppo_grad of mse_ppo.hip computes,
// for the same inputs and into the same slabs, with every product of a network on v_mfma_f32_32x32x2_f32 (f32 operands,
// f32 accumulation: an fmaf chain in another order).  DESIGN.md 4.12.  gfx950 only.
//
// A workgroup is four waves, as in k_ppo_grad: wave w runs the actor (w & 1 == 0) or the critic (w & 1 == 1) on tile slot
// w >> 1; a tile is 64 minibatch rows = two MFMA column tiles t = 0, 1 of 32 rows.  Layouts (lane l = (half h = l >> 5,
// j = l & 31)):
//   accumulator   register r of lane (h, j) of tile t: unit mat_row_of(r, h) of row 32 t + j.  It is the B operand of the
//                 next product's k-step r as it stands, because the weight image (mse_ppo_math.h: matrix_index) holds the
//                 A operands in that k order.  Forward layers, back-propagations and the element-wise arithmetic between
//                 them (ppo_tanh, 1 - h^2) never leave it.
//   row           lane l holds all AP logits of row l of the tile: the tile's logits go through the wave's LDS strip once
//                 ([64 rows][36]), policy_head_terms runs as it stands, the deltas go back the same way.
//   transposed    lane (h, u) holds unit u of rows 16 h .. 16 h + 15 of a column tile: both operands of a weight gradient
//                 delta^T x activation, whose k dimension is the rows.  Staged per layer and column tile in the strip as
//                 two [32 units][36] arrays, written from the accumulator layout, read back 16 bytes at a time.
// Weight-gradient accumulators (3 x 16 registers) stay in registers over all tiles of a wave; a bias gradient is the sum
// of the delta operands a lane reads, one register per layer, folded over the two halves at the end.  The critic's 32 -> 1
// head, its back-propagation and its weight gradient stay on the vector unit (a product one output wide).  The two waves of a
// network are added in a fixed order through LDS (slot 0 + slot 1) and the workgroup stores one slab.  No atomics.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>

#include "mse_ppo_grad.h"
#include "mse_ppo_math.h"

namespace {

using namespace mseppo;

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kStripStride = 36;                  // floats per staged row: 9 16-byte slots, odd, so 16 rows hit 16 slots
constexpr int kStripFloats = 64 * kStripStride;   // [64 rows][36] logits, or 2 x [32 units][36] transposed operands
constexpr int kTransposedFloats = 32 * kStripStride;
constexpr int kLdsFloats = kMatTotal + 4 * kStripFloats + kMiscFloats;
constexpr int kExchangeFloats = 51 * 64;          // per network: 3 x 16 accumulators + 3 bias sums of 64 lanes
static_assert(2 * kExchangeFloats <= 4 * kStripFloats, "the exchange reuses the strips");

// k-steps that cover units 0 .. n - 1 (n a multiple of 4): registers r with mat_row_of(r, 0) < n
constexpr int ksteps_for(int n)
{
    int k = 0;
    for (int r = 0; r < 16; ++r)
        if ((r & 3) + 8 * (r >> 2) < n) k = r + 1;
    return k;
}

// the value of the other half's lane j, added to this one's in the fixed order half 0 + half 1
__device__ __forceinline__ float halves_sum(float v)
{
    const uint32_t u = __float_as_uint(v);
    auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false); // {half 0's value, half 1's value} in every lane
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

__device__ __forceinline__ float4 lds4(const float *p) { return *reinterpret_cast<const float4 *>(p); }

// acc[t][r] = vec[mat_row_of(r, h)]: the same 16 bytes for every lane of a half (LDS broadcast)
__device__ __forceinline__ void vector_init(const float *vec, int h, f32x16 (&acc)[2])
{
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4 v = lds4(vec + 8 * g + 4 * h);
        const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[0][4 * g + q] = acc[1][4 * g + q] = e[q];
    }
}

// acc[t] += block x in[t] over KS k-steps; the A operands are read once and serve both column tiles
template <int KS>
__device__ __forceinline__ void product(const float *block, int lane, const float (&in)[2][16], f32x16 (&acc)[2])
{
#pragma unroll
    for (int g = 0; g < (KS + 3) / 4; ++g) {
        const float4 a4 = lds4(block + g * 256 + lane * 4); // [group][lane]: 16 bytes per lane, conflict-free
        const float a[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (4 * g + q < KS) {
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q], in[0][4 * g + q], acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q], in[1][4 * g + q], acc[1], 0, 0, 0);
            }
        }
    }
}

// acc[o][i] += sum over the tile's 64 rows of delta[o][row] act[i][row];  db += this lane's share of sum of delta[u = j]:
// rows 16 h .. 16 h + 15 of both column tiles.  Writes: lane (h, j) stores register r at [mat_row_of(r, h)][j], 32
// consecutive floats per half = 32 banks.  Reads: lane (h, u) takes 16-byte slot 9 u + 4 h + c of 16; a 16-lane group of
// ds_read_b128 lies in one half and holds every u mod 16 once, so its 16 slots are distinct.
__device__ __forceinline__ void weight_gradient(float *strip, int lane, const float (&delta)[2][16], const float (&act)[2][16],
                                                f32x16 &acc, float &db)
{
    const int h = lane >> 5, j = lane & 31;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        wave_lds_sync(); // whatever was read from the strip before has been read
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int at = ((r & 3) + 8 * (r >> 2) + 4 * h) * kStripStride + j;
            strip[at] = delta[t][r];
            strip[kTransposedFloats + at] = act[t][r];
        }
        wave_lds_sync();
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float4 d4 = lds4(strip + j * kStripStride + 16 * h + 4 * c);
            const float4 a4 = lds4(strip + kTransposedFloats + j * kStripStride + 16 * h + 4 * c);
            const float d[4] = {d4.x, d4.y, d4.z, d4.w}, a[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(d[q], a[q], acc, 0, 0, 0);
                db += d[q];
            }
        }
    }
}

struct LayerGrad {
    f32x16 w; // lane (h, i), register r: d loss / d W[mat_row_of(r, h)][i]
    float b;  // this lane's share of d loss / d b[j]
};

// one layer's accumulators -> the flat gradient: out[w_off + o * ld + i] (o < n_out, i < n_in), out[b_off + o]
__device__ __forceinline__ void store_layer(float *out, const LayerGrad &L, int lane, int w_off, int b_off, int n_out, int n_in, int ld)
{
    const int h = lane >> 5, j = lane & 31;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int o = (r & 3) + 8 * (r >> 2) + 4 * h;
        if (o < n_out && j < n_in) out[w_off + o * ld + j] = L.w[r];
    }
    const float b = halves_sum(L.b);
    if (h == 0 && j < n_out) out[b_off + j] = b;
}

// the critic's head, whose gradient is kept per lane (see the tile loop): out[w_off + u] = sum over the 32 lanes of the half
// that holds unit u, out[b_off] = sum over the wave; fixed butterflies
__device__ __forceinline__ void store_value_head(float *out, const LayerGrad &L, int lane, int w_off, int b_off)
{
    const int h = lane >> 5, j = lane & 31;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        float v = L.w[r];
#pragma unroll
        for (int m = 16; m > 0; m >>= 1) v += __shfl_xor(v, m, 64); // stays inside the half
        if (j == 0) out[w_off + (r & 3) + 8 * (r >> 2) + 4 * h] = v;
    }
    const float b = wave_sum(L.b);
    if (lane == 0) out[b_off] = b;
}

// VCLIP: SB3's clip_range_vf (value_head_terms_clipped on old_values[row]); false never reads old_values
// BC: behaviour cloning, as in k_ppo_grad: bc_head_terms on the demonstrated action with the sums ce, entropy, hits, unusable;
// old_logp, adv and adv_partial are never read; with ret == NULL the critic's waves take no tile.  false: the kernel as it was.
template <int DP, int AP, bool VCLIP, bool BC = false>
__global__ __launch_bounds__(256) void k_ppo_grad_matrix(GradArgs G, const float *__restrict__ weights,
                                                         const long long *__restrict__ rows, const float *__restrict__ obs,
                                                         const uint8_t *__restrict__ mask, const int *__restrict__ actions,
                                                         const float *__restrict__ old_logp, const float *__restrict__ adv,
                                                         const float *__restrict__ ret, const double *__restrict__ adv_partial,
                                                         float *__restrict__ slabs, const int *__restrict__ control,
                                                         const float *__restrict__ old_values)
{
    // the body needs: DP, AP, VCLIP, BC (template parameters), KICK, K, SHARD, S and the arguments above
    constexpr bool KICK = false, SHARD = false;
    [[maybe_unused]] const KickArgs K{nullptr, 0.0f};
    [[maybe_unused]] const ShardArgs S{0, nullptr};
#include "mse_ppo_matrix_body.inc"
}

// KICK: PPO with an imitation term, as in k_ppo_grad_kick: policy_bc_head_terms on K.expert_actions[row] with K.bc_coef, seven
// sums, slab_stride_kick, kKickMiscFloats; everything else is the same statements (mse_ppo_matrix_body.inc)
template <int DP, int AP, bool VCLIP>
__global__ __launch_bounds__(256) void k_ppo_grad_matrix_kick(GradArgs G, const float *__restrict__ weights,
                                                              const long long *__restrict__ rows, const float *__restrict__ obs,
                                                              const uint8_t *__restrict__ mask, const int *__restrict__ actions,
                                                              const float *__restrict__ old_logp, const float *__restrict__ adv,
                                                              const float *__restrict__ ret, const double *__restrict__ adv_partial,
                                                              float *__restrict__ slabs, const int *__restrict__ control,
                                                              const float *__restrict__ old_values, KickArgs K)
{
    // the body needs: DP, AP, VCLIP (template parameters), BC, KICK, K, SHARD, S and the arguments above
    constexpr bool BC = false, KICK = true, SHARD = false;
    [[maybe_unused]] const ShardArgs S{0, nullptr};
#include "mse_ppo_matrix_body.inc"
}

// SHARD: one shard of a minibatch, as in k_ppo_grad_shard: G.batch local rows, per-row terms scaled by 1 / S.global_batch, the
// advantage mean and std from S.moments; everything else is the same statements (mse_ppo_matrix_body.inc)
template <int DP, int AP, bool VCLIP>
__global__ __launch_bounds__(256) void k_ppo_grad_matrix_shard(GradArgs G, const float *__restrict__ weights,
                                                               const long long *__restrict__ rows, const float *__restrict__ obs,
                                                               const uint8_t *__restrict__ mask, const int *__restrict__ actions,
                                                               const float *__restrict__ old_logp, const float *__restrict__ adv,
                                                               const float *__restrict__ ret, float *__restrict__ slabs,
                                                               const int *__restrict__ control, const float *__restrict__ old_values,
                                                               ShardArgs S)
{
    // the body needs: DP, AP, VCLIP (template parameters), BC, KICK, K, SHARD, S and the arguments above
    constexpr bool BC = false, KICK = false, SHARD = true;
    [[maybe_unused]] const KickArgs K{nullptr, 0.0f};
    [[maybe_unused]] const double *adv_partial = nullptr; // named by the branch SHARD discards
#include "mse_ppo_matrix_body.inc"
}

// the image and the four strips take more than the 64 KB a launch gets unasked: once per kernel and device (set twice at worst)
hipError_t allow_lds(const void *kernel, size_t lds, std::atomic<bool> (&allowed)[64])
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return hipErrorNoDevice;
    if (dev < 0 || dev >= 64 || !allowed[dev].load(std::memory_order_relaxed)) {
        const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        if (dev >= 0 && dev < 64) allowed[dev].store(true, std::memory_order_relaxed);
    }
    return hipSuccess;
}

template <int DP, int AP, bool VCLIP, bool BC = false>
hipError_t launch(const GradArgs &G, int n_slabs, hipStream_t s, const float *weights, const long long *rows, const float *obs,
                  const uint8_t *mask, const int *actions, const float *old_logp, const float *adv, const float *ret,
                  const double *adv_partial, float *slabs, const int *control, const float *old_values)
{
    constexpr size_t lds = (size_t)kLdsFloats * sizeof(float);
    static std::atomic<bool> allowed[64];
    const hipError_t e = allow_lds(reinterpret_cast<const void *>(&k_ppo_grad_matrix<DP, AP, VCLIP, BC>), lds, allowed);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_ppo_grad_matrix<DP, AP, VCLIP, BC>), dim3((unsigned)n_slabs), dim3(256), lds, s, G, weights, rows, obs, mask,
                       actions, old_logp, adv, ret, adv_partial, slabs, control, old_values);
    return hipGetLastError();
}

template <int DP, int AP, bool VCLIP>
hipError_t launch_kick(const GradArgs &G, int n_slabs, hipStream_t s, const float *weights, const long long *rows, const float *obs,
                       const uint8_t *mask, const int *actions, const float *old_logp, const float *adv, const float *ret,
                       const double *adv_partial, float *slabs, const int *control, const float *old_values, const KickArgs &K)
{
    constexpr size_t lds = (size_t)(kLdsFloats - kMiscFloats + kKickMiscFloats) * sizeof(float);
    static std::atomic<bool> allowed[64];
    const hipError_t e = allow_lds(reinterpret_cast<const void *>(&k_ppo_grad_matrix_kick<DP, AP, VCLIP>), lds, allowed);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_ppo_grad_matrix_kick<DP, AP, VCLIP>), dim3((unsigned)n_slabs), dim3(256), lds, s, G, weights, rows, obs, mask,
                       actions, old_logp, adv, ret, adv_partial, slabs, control, old_values, K);
    return hipGetLastError();
}

template <int DP, int AP, bool VCLIP>
hipError_t launch_shard(const GradArgs &G, int n_slabs, hipStream_t s, const float *weights, const long long *rows, const float *obs,
                        const uint8_t *mask, const int *actions, const float *old_logp, const float *adv, const float *ret, float *slabs,
                        const int *control, const float *old_values, const ShardArgs &S)
{
    constexpr size_t lds = (size_t)kLdsFloats * sizeof(float);
    static std::atomic<bool> allowed[64];
    const hipError_t e = allow_lds(reinterpret_cast<const void *>(&k_ppo_grad_matrix_shard<DP, AP, VCLIP>), lds, allowed);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_ppo_grad_matrix_shard<DP, AP, VCLIP>), dim3((unsigned)n_slabs), dim3(256), lds, s, G, weights, rows, obs, mask,
                       actions, old_logp, adv, ret, slabs, control, old_values, S);
    return hipGetLastError();
}

} // namespace

hipError_t mse_ppo_launch_grad_matrix_shard(const GradArgs &G, int n_slabs, hipStream_t stream, const float *weights,
                                            const long long *rows, const float *obs, const uint8_t *mask, const int *actions,
                                            const float *old_logp, const float *adv, const float *ret, float *slabs,
                                            const int *control, const float *old_values, const ShardArgs &S)
{
    hipError_t e = hipErrorInvalidValue;
#define MSE_SHARD_MATRIX_LAUNCH(DP, AP)                                                                                              \
    e = old_values != nullptr                                                                                                        \
            ? launch_shard<DP, AP, true>(G, n_slabs, stream, weights, rows, obs, mask, actions, old_logp, adv, ret, slabs, control, \
                                         old_values, S)                                                                              \
            : launch_shard<DP, AP, false>(G, n_slabs, stream, weights, rows, obs, mask, actions, old_logp, adv, ret, slabs, control, \
                                          old_values, S)
    MSE_PPO_DISPATCH(select_grad_shape(G.D, G.A), MSE_SHARD_MATRIX_LAUNCH);
#undef MSE_SHARD_MATRIX_LAUNCH
    return e;
}

hipError_t mse_ppo_launch_grad_matrix(const GradArgs &G, int n_slabs, hipStream_t stream, const float *weights,
                                      const long long *rows, const float *obs, const uint8_t *mask, const int *actions,
                                      const float *old_logp, const float *adv, const float *ret, const double *adv_partial,
                                      float *slabs, const int *control, const float *old_values)
{
    hipError_t e = hipErrorInvalidValue;
    // the four padded shapes of k_ppo_grad, chosen by the same function
#define MSE_PPO_MATRIX_LAUNCH(DP, AP)                                                                                                \
    e = old_values != nullptr                                                                                                        \
            ? launch<DP, AP, true>(G, n_slabs, stream, weights, rows, obs, mask, actions, old_logp, adv, ret, adv_partial, slabs,   \
                                   control, old_values)                                                                              \
            : launch<DP, AP, false>(G, n_slabs, stream, weights, rows, obs, mask, actions, old_logp, adv, ret, adv_partial, slabs,  \
                                    control, old_values)
    MSE_PPO_DISPATCH(select_grad_shape(G.D, G.A), MSE_PPO_MATRIX_LAUNCH);
#undef MSE_PPO_MATRIX_LAUNCH
    return e;
}

hipError_t mse_ppo_launch_grad_matrix_bc(const GradArgs &G, int n_slabs, hipStream_t stream, const float *weights,
                                         const long long *rows, const float *obs, const uint8_t *mask, const int *actions,
                                         const float *ret, float *slabs)
{
    hipError_t e = hipErrorInvalidValue;
#define MSE_BC_MATRIX_LAUNCH(DP, AP)                                                                                              \
    e = launch<DP, AP, false, true>(G, n_slabs, stream, weights, rows, obs, mask, actions, nullptr, nullptr, ret, nullptr, slabs, \
                                    nullptr, nullptr)
    MSE_PPO_DISPATCH(select_grad_shape(G.D, G.A), MSE_BC_MATRIX_LAUNCH);
#undef MSE_BC_MATRIX_LAUNCH
    return e;
}

hipError_t mse_ppo_launch_grad_matrix_kick(const GradArgs &G, int n_slabs, hipStream_t stream, const float *weights,
                                           const long long *rows, const float *obs, const uint8_t *mask, const int *actions,
                                           const float *old_logp, const float *adv, const float *ret, const double *adv_partial,
                                           float *slabs, const int *control, const float *old_values, const KickArgs &K)
{
    hipError_t e = hipErrorInvalidValue;
#define MSE_KICK_MATRIX_LAUNCH(DP, AP)                                                                                                  \
    e = old_values != nullptr                                                                                                           \
            ? launch_kick<DP, AP, true>(G, n_slabs, stream, weights, rows, obs, mask, actions, old_logp, adv, ret, adv_partial, slabs, \
                                        control, old_values, K)                                                                         \
            : launch_kick<DP, AP, false>(G, n_slabs, stream, weights, rows, obs, mask, actions, old_logp, adv, ret, adv_partial, slabs, \
                                         control, old_values, K)
    MSE_PPO_DISPATCH(select_grad_shape(G.D, G.A), MSE_KICK_MATRIX_LAUNCH);
#undef MSE_KICK_MATRIX_LAUNCH
    return e;
}
