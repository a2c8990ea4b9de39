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
    constexpr int KS1 = DP / 2;          // k-steps of the first layer: units 0 .. DP - 1
    constexpr int KSA = ksteps_for(AP);  // k-steps of the head's back-propagation: actions 0 .. AP - 1
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int D = G.D, A = G.A;
    const Flat F = flat_layout(D, A);
    if (gate_closed(control)) { // grid-uniform
        mark_gate_closed(F.total, slabs);
        return;
    }
    float *wl0 = lds;                       // kMatTotal floats: the operand image
    float *strips = lds + kMatTotal;        // 4 x kStripFloats: one staging strip per wave
    float *misc = strips + 4 * kStripFloats; // kMiscFloats
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = lane >> 5, j = lane & 31;
    for (int i = tid; i < kMatTotal; i += 256) wl0[i] = 0.0f;
    __syncthreads();
    for (int f = tid; f < F.total; f += 256) {
        const float w = weights[f];
        wl0[matrix_index(f, D, A)] = w;
        const int tr = matrix_index_transposed(f, D, A);
        if (tr >= 0) wl0[tr] = w;
    }
    publish_adv_mean_std(G, rows, adv, adv_partial, misc, wave, lane);
    __syncthreads();
    const bool normalize = G.n_adv_partial > 0;
    const float mean = misc[0], std = misc[1];
    const float inv_b_all = 1.0f / (float)G.batch;
    const bool critic = (wave & 1) != 0;
    float *strip = strips + wave * kStripFloats;
    LayerGrad L1, L2, L3; // first, second hidden layer, head
#pragma unroll
    for (int r = 0; r < 16; ++r) L1.w[r] = L2.w[r] = L3.w[r] = 0.0f;
    L1.b = L2.b = L3.b = 0.0f;
    float st0 = 0.0f, st1 = 0.0f, st2 = 0.0f, st3 = 0.0f;
    long long n_tiles = (G.batch + 63) / 64;
    if constexpr (BC) n_tiles = critic && ret == nullptr ? 0 : n_tiles; // wave-uniform: no returns, nothing for the critic
    for (long long tile = (long long)blockIdx.x * 2 + (wave >> 1); tile < n_tiles; tile += (long long)gridDim.x * 2) {
        // the image is re-read from LDS every tile: an offset the compiler cannot see through keeps it from hoisting the
        // operands of one tile's products out of the loop into registers it does not have
        unsigned opaque = 0;
        asm volatile("" : "+v"(opaque));
        const float *wl = static_cast<const float *>(__builtin_assume_aligned(wl0 + 4 * opaque, 16));
        // the two rows this lane meets in the accumulator layout (column j of both column tiles); its own row in the row
        // layout is the one of column tile h
        long long row_t[2];
        float inv_b_t[2];
        bool valid_t[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const long long b = tile * 64 + 32 * t + j;
            valid_t[t] = b < G.batch;
            row_t[t] = row_at(rows, valid_t[t] ? b : 0, G.n_rows);
            inv_b_t[t] = valid_t[t] ? inv_b_all : 0.0f; // a padding row contributes zero deltas
        }
        float x[2][16];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                const int u = (s & 3) + 8 * (s >> 2) + 4 * h;
                x[t][s] = 0.0f;
                if (s < KS1) {
                    const float v = obs[row_t[t] * D + (u < D ? u : 0)];
                    x[t][s] = u < D ? v : 0.0f;
                }
            }
        }
        float h1[2][16], h2[2][16], d[2][16];
        f32x16 acc[2];
        vector_init(wl + (critic ? kMatVfB1 : kMatPiB1), h, acc);
        product<KS1>(wl + (critic ? kMatVfW1 : kMatPiW1) * kMatBlockFloats, lane, x, acc);
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) h1[t][r] = ppo_tanh(acc[t][r]);
        vector_init(wl + (critic ? kMatVfB2 : kMatPiB2), h, acc);
        product<16>(wl + (critic ? kMatVfW2 : kMatPiW2) * kMatBlockFloats, lane, h1, acc);
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) h2[t][r] = ppo_tanh(acc[t][r]);
        if (!critic) {
            vector_init(wl + kMatActB, h, acc);
            product<16>(wl + kMatActW * kMatBlockFloats, lane, h2, acc);
            // logits: accumulator layout -> row layout.  Writes are 16-byte words at slot 9 j + const of 8 (8 consecutive
            // lanes of a half per group: distinct); reads at slot 9 l + c of 16 (every l mod 16 once per group).
            wave_lds_sync();
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    if (8 * g < AP)
                        *reinterpret_cast<float4 *>(strip + (32 * t + j) * kStripStride + 8 * g + 4 * h) =
                            make_float4(acc[t][4 * g], acc[t][4 * g + 1], acc[t][4 * g + 2], acc[t][4 * g + 3]);
            wave_lds_sync();
            const long long row = h ? row_t[1] : row_t[0];
            const bool valid = h ? valid_t[1] : valid_t[0];
            const float inv_b = h ? inv_b_t[1] : inv_b_t[0];
            float dl[AP];
#pragma unroll
            for (int c = 0; c < AP / 4; ++c) {
                const float4 v = lds4(strip + lane * kStripStride + 4 * c);
                dl[4 * c] = v.x;
                dl[4 * c + 1] = v.y;
                dl[4 * c + 2] = v.z;
                dl[4 * c + 3] = v.w;
            }
            uint32_t legal = 0;
#pragma unroll
            for (int a = 0; a < AP; ++a) {
                const bool ok = a < A && (mask == nullptr || mask[row * A + (a < A ? a : 0)] != 0);
                legal |= (ok ? 1u : 0u) << a;
            }
            if constexpr (BC) {
                const BcTerms bt = bc_head_terms<AP>(dl, A, legal, actions[row], G.P, inv_b);
                if (valid) {
                    st0 += bt.ce;
                    st1 += bt.entropy;
                    st2 += bt.hit;
                    st3 += bt.unusable;
                }
            } else {
                const int action = clamped_action(actions[row], A);
                const float a_raw = adv[row];
                const float a_used = normalize ? normalized_advantage(a_raw, mean, std) : a_raw;
                const PolicyTerms pt = policy_head_terms<AP>(dl, A, legal, action, old_logp[row], a_used, G.P, inv_b);
                if (valid) {
                    st0 += pt.surrogate;
                    st1 += pt.entropy;
                    st2 += pt.kl;
                    st3 += pt.clipped;
                }
            }
            // deltas: row layout -> accumulator layout (a lane overwrites the row it read; actions AP .. 31 are zero)
#pragma unroll
            for (int c = 0; c < AP / 4; ++c)
                *reinterpret_cast<float4 *>(strip + lane * kStripStride + 4 * c) = make_float4(dl[4 * c], dl[4 * c + 1], dl[4 * c + 2], dl[4 * c + 3]);
            wave_lds_sync();
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    if (8 * g < AP) {
                        v = lds4(strip + (32 * t + j) * kStripStride + 8 * g + 4 * h);
                        if (8 * g + 4 >= AP && h != 0) v = make_float4(0.0f, 0.0f, 0.0f, 0.0f); // half 1's words start at 8 g + 4
                    }
                    d[t][4 * g] = v.x;
                    d[t][4 * g + 1] = v.y;
                    d[t][4 * g + 2] = v.z;
                    d[t][4 * g + 3] = v.w;
                }
            weight_gradient(strip, lane, d, h2, L3.w, L3.b);
            acc[0] = acc[1] = 0.0f;
            product<KSA>(wl + kMatActWT * kMatBlockFloats, lane, d, acc);
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) d[t][r] = acc[t][r] * fmaf(-h2[t][r], h2[t][r], 1.0f);
        } else {
            // the 32 -> 1 head and its back-propagation on the vector unit: a lane has 16 of a row's 32 units
            float vw[16];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 v = lds4(wl + kMatValW + 8 * g + 4 * h);
                vw[4 * g] = v.x;
                vw[4 * g + 1] = v.y;
                vw[4 * g + 2] = v.z;
                vw[4 * g + 3] = v.w;
            }
            const float vb = wl[kMatValB];
            float dv[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                float part = 0.0f;
#pragma unroll
                for (int r = 0; r < 16; ++r) part = fmaf(vw[r], h2[t][r], part);
                const float value = halves_sum(part) + vb;
                float sq;
                if constexpr (VCLIP)
                    sq = value_head_terms_clipped(value, old_values[row_t[t]], ret[row_t[t]], G.P, inv_b_t[t], dv[t]);
                else
                    sq = value_head_terms(value, ret[row_t[t]], G.P, inv_b_t[t], dv[t]);
                if (valid_t[t] && h == t) st0 += sq; // both halves hold the row: half t counts it
                // the head's weight gradient, one output wide, stays here too: L3.w[r] is this lane's share (column j of
                // both column tiles) of d loss / d val_w[mat_row_of(r, h)], summed over the half's lanes at the end
#pragma unroll
                for (int r = 0; r < 16; ++r) L3.w[r] = fmaf(dv[t], h2[t][r], L3.w[r]);
                if (h == t) L3.b += dv[t];
            }
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) d[t][r] = fmaf(vw[r], dv[t], 0.0f) * fmaf(-h2[t][r], h2[t][r], 1.0f);
        }
        weight_gradient(strip, lane, d, h1, L2.w, L2.b);
        acc[0] = acc[1] = 0.0f;
        product<16>(wl + (critic ? kMatVfW2T : kMatPiW2T) * kMatBlockFloats, lane, d, acc);
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) d[t][r] = acc[t][r] * fmaf(-h1[t][r], h1[t][r], 1.0f);
        weight_gradient(strip, lane, d, x, L1.w, L1.b);
    }
    // ---- the two waves of a network: slot 1 hands its sums to slot 0 through LDS; fixed order (slot 0 + slot 1) ----
    st0 = wave_sum(st0);
    st1 = wave_sum(st1);
    st2 = wave_sum(st2);
    st3 = wave_sum(st3);
    __syncthreads(); // every wave is done with its strip
    float *xch = strips + (wave & 1) * kExchangeFloats;
    if (wave >= 2) {
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            xch[(k)*64 + lane] = L1.w[k];
            xch[(16 + k) * 64 + lane] = L2.w[k];
            xch[(32 + k) * 64 + lane] = L3.w[k];
        }
        xch[48 * 64 + lane] = L1.b;
        xch[49 * 64 + lane] = L2.b;
        xch[50 * 64 + lane] = L3.b;
    }
    publish_loss_sums(misc, wave, lane, st0, st1, st2, st3);
    __syncthreads();
    float *slab = slabs + (long long)blockIdx.x * slab_stride(F.total);
    if (wave < 2) {
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            L1.w[k] += xch[(k)*64 + lane];
            L2.w[k] += xch[(16 + k) * 64 + lane];
            L3.w[k] += xch[(32 + k) * 64 + lane];
        }
        L1.b += xch[48 * 64 + lane];
        L2.b += xch[49 * 64 + lane];
        L3.b += xch[50 * 64 + lane];
        if (!critic) {
            store_layer(slab, L1, lane, F.pi_w1, F.pi_b1, kH, D, D);
            store_layer(slab, L2, lane, F.pi_w2, F.pi_b2, kH, kH, kH);
            store_layer(slab, L3, lane, F.act_w, F.act_b, A, kH, kH);
        } else {
            store_layer(slab, L1, lane, F.vf_w1, F.vf_b1, kH, D, D);
            store_layer(slab, L2, lane, F.vf_w2, F.vf_b2, kH, kH, kH);
            store_value_head(slab, L3, lane, F.val_w, F.val_b);
        }
    }
    if (tid == 0) store_slab_stats(slab + F.total, misc);
}

template <int DP, int AP, bool VCLIP, bool BC = false>
hipError_t launch(const GradArgs &G, int n_slabs, hipStream_t s, const float *weights, const long long *rows, const float *obs,
                  const uint8_t *mask, const int *actions, const float *old_logp, const float *adv, const float *ret,
                  const double *adv_partial, float *slabs, const int *control, const float *old_values)
{
    constexpr size_t lds = (size_t)kLdsFloats * sizeof(float);
    // the image and the four strips take more than the 64 KB a launch gets unasked
    static std::atomic<bool> allowed[64]; // per device; set twice at worst
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return hipErrorNoDevice;
    if (dev < 0 || dev >= 64 || !allowed[dev].load(std::memory_order_relaxed)) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_ppo_grad_matrix<DP, AP, VCLIP, BC>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        if (dev >= 0 && dev < 64) allowed[dev].store(true, std::memory_order_relaxed);
    }
    hipLaunchKernelGGL((k_ppo_grad_matrix<DP, AP, VCLIP, BC>), dim3((unsigned)n_slabs), dim3(256), lds, s, G, weights, rows, obs, mask,
                       actions, old_logp, adv, ret, adv_partial, slabs, control, old_values);
    return hipGetLastError();
}

} // namespace

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
