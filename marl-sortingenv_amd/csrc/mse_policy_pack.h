// mse_policy_pack.h -- torch.nn.Linear weights -> the packed image the policy kernels read (mse_policy_device.h), in
// plain C++ that compiles for the host and for the device alike (as mse_ppo_math.h and mse_episode_math.h do): the host
// packer (pack_weights, mse_policy_pack_host) and the device repack (k_policy_pack) of mse_policy.hip run these
// functions, so the two produce the same bytes and tests/test_policy_pack_cpu.py can hold the arithmetic against
// tests/policy_pack_reference.py without a GPU.  The library is built with -ffp-contract=off: every operation below is
// rounded on its own, on both sides.
//
// Input: the flat weights f32[W] in the order of include/mse.h, H = 32:
//   pi_w1[H*D] pi_b1[H] pi_w2[H*H] pi_b2[H] act_w[A*H] act_b[A] vf_w1[H*D] vf_b1[H] vf_w2[H*H] vf_b2[H] val_w[H] val_b[1]
// matrices row-major [out, in].
//
// 1. The fold, in float64 (c = 2 log2 e = 2.0 * 1.4426950408889634, a hidden unit is r = 1 / (2^z + 1), tanh = 1 - 2 r,
//    so a layer fed by r instead of tanh is  W tanh + b = (b + W 1) + (-2 W) r).  Dense 32 x 32 matrices Wf[L][out][in]
//    and biases Bf[L][out] for the layers L = 0 actor-1, 1 actor-2, 2 action head, 3 critic-1, 4 critic-2; x means the
//    f32 weight converted to double; cells the formulas do not reach (in >= D, head out >= A) are +0.0:
//      Wf[0][o][i] = c * pi_w1[o, i]            Bf[0][o] = c * pi_b1[o]                                   (3: vf_w1, vf_b1)
//      Wf[1][o][i] = (-2.0 * c) * pi_w2[o, i]   Bf[1][o] = c * (pi_b2[o] + S),  S = sum_i pi_w2[o, i]     (4: vf_w2, vf_b2)
//      Wf[2][o][i] = -2.0 * act_w[o, i]         Bf[2][o] = act_b[o] + S,        S = sum_i act_w[o, i]
//      value head:  wv[i] = -2.0 * val_w[i],    bv = val_b[0] + S,              S = sum_i val_w[i]
//    Every S starts at 0.0 and adds i = 0, 1, .. 31 in that order, one double add each.  Every result is then rounded to
//    f32 once (round to nearest even); the rest works on those f32 values.
//
// 2. The operand order.  row_of(r, h) = (r & 3) + 8 * (r >> 2) + 4 * h is the row accumulator register r holds in lane
//    half h.  MFMA k-step s (0 .. 15) of lane l = 32 * hp + i multiplies output row i by input
//      k = 2 * s + hp        in the input layers 0 and 3 (the observation comes in natural order),
//      k = row_of(s, hp)     in layers 1, 2 and 4 (the previous layer's accumulator registers are the B operands).
//
// 3. The image, kBlobFloats f32 cells (offsets in mse_policy_device.h):
//      [kOffB  + (2 * L + h) * 16 + r]                     = f32(Bf[L][row_of(r, h)])           L < 5, h < 2, r < 16
//      [kOffWV + h * 16 + r]                               = f32(wv[row_of(r, h)])
//      [kOffBV]                                            = f32(bv);   the cells up to kOffW are +0.0
//      [kOffW  + ((4 * L + (s >> 2)) * 64 + l) * 4 + (s & 3)] = wf = f32(Wf[L][i][k])           the f32 operands
//      from kOffW16 on, 16-bit cells:  hi at  ((2 * L + (s >> 3)) * 64 + l) * 8 + (s & 7),  lo 5 * 2 * 64 * 8 cells later
//        hi = half_rtz(wf),   lo = half_rne(wf - f32(hi))   (the subtraction in f32; it is exact)
//    The f16 section is specified only when f16_ok = every |wf| < 65504 (a NaN fails); its content is unspecified
//    otherwise, and the rest of the image never depends on it.
//
// 4. half_rtz(v), on the bits of the f32 v (sign sg, biased exponent field E, e = E - 127, m = mantissa | 2^23):
//      E == 0 (zero, f32 subnormal)   ->  sg                                  (signed zero)
//      e >= -14                       ->  sg | (e + 15) << 10 | (m >> 13) & 0x3FF
//      -25 <= e < -14                 ->  sg | m >> (13 + (-14 - e))          (f16 subnormal: the mantissa shifted out)
//      e < -25                        ->  sg
//    half_rne(v): t = half_rtz(v), u = t + 1 (the next magnitude of the same sign); with a, b the values of t and u,
//    da = |v - a|, db = |b - v|: the result is u if db < da, or if db == da and u is even, else t.  Both differences are
//    exact in f32 except far below the f16 subnormal step, where their order is unaffected.
#pragma once

#include <stdint.h>

#include "mse_policy_device.h"

#if defined(__HIPCC__)
#define MSE_PK_HD __host__ __device__ __forceinline__
#else
#define MSE_PK_HD inline
#endif

namespace msepack {

using msep::kBlobFloats;
using msep::kHidden;
using msep::kOffB;
using msep::kOffBV;
using msep::kOffW;
using msep::kOffW16;
using msep::kOffWV;
using msep::row_of;

constexpr int kOperandCells = 5 * 16 * 64;  // operands per form: [layer][k-step][lane]
constexpr int kOperandGroups = 5 * 4 * 64;  // groups of four consecutive k-steps of one lane = one 16-byte f32 word
constexpr float kHalfLimit = 65504.0f;      // the f16x3 form needs every |folded weight| below this

struct Flat {
    int pi_w1, pi_b1, pi_w2, pi_b2, act_w, act_b, vf_w1, vf_b1, vf_w2, vf_b2, val_w, val_b, total;
};

MSE_PK_HD Flat flat_offsets(int D, int A)
{
    const int H = kHidden;
    Flat F;
    F.pi_w1 = 0;
    F.pi_b1 = F.pi_w1 + H * D;
    F.pi_w2 = F.pi_b1 + H;
    F.pi_b2 = F.pi_w2 + H * H;
    F.act_w = F.pi_b2 + H;
    F.act_b = F.act_w + A * H;
    F.vf_w1 = F.act_b + A;
    F.vf_b1 = F.vf_w1 + H * D;
    F.vf_w2 = F.vf_b1 + H;
    F.vf_b2 = F.vf_w2 + H * H;
    F.val_w = F.vf_b2 + H;
    F.val_b = F.val_w + H;
    F.total = F.val_b + 1;
    return F;
}

constexpr double kFoldC = 2.0 * 1.4426950408889634073599246810019;

// S = sum of 32 consecutive weights, i = 0 .. 31 in order, in double
MSE_PK_HD double row_sum(const float *row)
{
    double s = 0.0;
    for (int i = 0; i < kHidden; ++i) s += (double)row[i];
    return s;
}

// Wf[L][o][i], o and i in 0 .. 31
MSE_PK_HD double folded_weight(const float *w, const Flat &F, int D, int A, int L, int o, int i)
{
    const int H = kHidden;
    const double c = kFoldC;
    switch (L) {
    case 0: return i < D ? c * (double)w[F.pi_w1 + o * D + i] : 0.0;
    case 3: return i < D ? c * (double)w[F.vf_w1 + o * D + i] : 0.0;
    case 1: return -2.0 * c * (double)w[F.pi_w2 + o * H + i];
    case 4: return -2.0 * c * (double)w[F.vf_w2 + o * H + i];
    default: return o < A ? -2.0 * (double)w[F.act_w + o * H + i] : 0.0;
    }
}

// Bf[L][o]
MSE_PK_HD double folded_bias(const float *w, const Flat &F, int A, int L, int o)
{
    const int H = kHidden;
    const double c = kFoldC;
    switch (L) {
    case 0: return c * (double)w[F.pi_b1 + o];
    case 3: return c * (double)w[F.vf_b1 + o];
    case 1: return c * ((double)w[F.pi_b2 + o] + row_sum(w + F.pi_w2 + o * H));
    case 4: return c * ((double)w[F.vf_b2 + o] + row_sum(w + F.vf_w2 + o * H));
    default: return o < A ? (double)w[F.act_b + o] + row_sum(w + F.act_w + o * H) : 0.0;
    }
}

// cell `idx` of the image's head [0, kOffW): biases, value head, padding
MSE_PK_HD float head_cell(const float *w, const Flat &F, int A, int idx)
{
    if (idx < kOffWV) {
        const int j = idx - kOffB;
        return (float)folded_bias(w, F, A, j >> 5, row_of(j & 15, (j >> 4) & 1));
    }
    if (idx < kOffBV) {
        const int j = idx - kOffWV;
        return (float)(-2.0 * (double)w[F.val_w + row_of(j & 15, j >> 4)]);
    }
    if (idx == kOffBV) return (float)((double)w[F.val_b] + row_sum(w + F.val_w));
    return 0.0f;
}

// the f32 operand of layer L, k-step s, lane l
MSE_PK_HD float operand(const float *w, const Flat &F, int D, int A, int L, int s, int lane)
{
    const int hp = lane >> 5;
    const int k = (L == 0 || L == 3) ? 2 * s + hp : row_of(s, hp);
    return (float)folded_weight(w, F, D, A, L, lane & 31, k);
}

MSE_PK_HD int f32_cell(int L, int s, int lane) { return kOffW + ((L * 4 + (s >> 2)) * 64 + lane) * 4 + (s & 3); }
MSE_PK_HD int f16_cell(int L, int s, int lane) { return ((L * 2 + (s >> 3)) * 64 + lane) * 8 + (s & 7); } // hi; lo: + kOperandCells

MSE_PK_HD bool fits_half(float wf) { return __builtin_fabsf(wf) < kHalfLimit; }

MSE_PK_HD float f32_of_half(uint16_t hb)
{
    const uint32_t sgn = (uint32_t)(hb & 0x8000u) << 16, ex = (hb >> 10) & 0x1Fu, man = hb & 0x3FFu;
    if (ex == 0) return (sgn ? -1.0f : 1.0f) * ((float)man * 0x1p-24f); // exact: man < 2^10
    return __builtin_bit_cast(float, sgn | ((ex + 112u) << 23) | (man << 13));
}

MSE_PK_HD uint16_t half_rtz(float v) // f32 -> f16, round toward zero, subnormals kept, |v| < 65520
{
    const uint32_t u = __builtin_bit_cast(uint32_t, v);
    const uint16_t sgn = (uint16_t)((u >> 16) & 0x8000u);
    const int ex = (int)((u >> 23) & 0xFFu) - 127;
    const uint32_t man = (u & 0x7FFFFFu) | 0x800000u;
    if (((u >> 23) & 0xFFu) == 0) return sgn; // f32 zero / subnormal
    if (ex >= -14) return (uint16_t)(sgn | ((uint32_t)(ex + 15) << 10) | ((man >> 13) & 0x3FFu));
    if (ex < -25) return sgn;
    return (uint16_t)(sgn | (man >> (13 + (-14 - ex)))); // subnormal: shift the mantissa out
}

MSE_PK_HD uint16_t half_rne(float v) // to nearest: the truncated value or its successor, whichever is closer
{
    const uint16_t lo_b = half_rtz(v);
    const uint16_t hi_b = (uint16_t)(lo_b + 1); // next magnitude (same sign); fine below the largest finite half
    const float a = f32_of_half(lo_b), b = f32_of_half(hi_b);
    const float da = __builtin_fabsf(v - a), db = __builtin_fabsf(b - v);
    return (db < da || (db == da && (hi_b & 1u) == 0)) ? hi_b : lo_b;
}

struct HalfPair {
    uint16_t hi, lo;
};
MSE_PK_HD HalfPair split_half(float wf)
{
    HalfPair p;
    p.hi = half_rtz(wf);
    p.lo = half_rne(wf - f32_of_half(p.hi));
    return p;
}

} // namespace msepack
