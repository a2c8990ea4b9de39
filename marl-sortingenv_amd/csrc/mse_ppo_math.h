// mse_ppo_math.h -- the per-row arithmetic of the on-device PPO learner (mse_ppo.hip), in plain C++ that compiles for
// the host and for the device alike (as mse_exact.h and mse_plan.h do), so tests/test_ppo_math_cpu.py can hold it
// against float64 autograd without a GPU.
//
// What it restates (stable-baselines3 / sb3-contrib, which src/training.py:115-131,191 of the reference drives):
//   gae_column          RolloutBuffer.compute_returns_and_advantage, one env, every operation separately rounded
//   policy_head_terms   MaskableCategorical (illegal logits at -1e8), log-prob / entropy, the clipped surrogate of
//                       MaskablePPO.train and the gradient of  policy_loss + ent_coef * entropy_loss  w.r.t. the logits
//   bc_head_terms       behaviour cloning: the cross-entropy of a demonstrated action under the same masked softmax, its
//                       accuracy / unusable-row counts and the gradient of  ce + ent_coef * entropy_loss  (restates no SB3 code)
//   policy_bc_head_terms  PPO with an auxiliary imitation term: policy_head_terms and bc_head_terms on one masked softmax, the
//                       gradient of  policy_loss + ent_coef * entropy_loss + bc_coef * ce  (DAPG / kickstarting; no SB3 code)
//   value_head_terms    F.mse_loss(returns, values) and its gradient
//   value_head_terms_clipped   the same for PPO.train's clip_range_vf: values clipped to within c of the rollout's
//   ev_groups / ev_lane_sums / ev_from_sums   explained_variance(values, returns), the sums and their order in full
//   hidden_forward / head_forward / backprop            the 2 x 32 tanh MLP and the deltas of its layers
// and, restating nothing (SB3 shuffles with numpy's generator):
//   shuffle_key / shuffle_index   the counter-based permutation of an epoch's rows, specified in full where it is defined
// The weights are read from a PADDED image (Padded<DP, AP>: rows of the first layer padded to DP inputs, the action
// head to AP rows, zeros in the padding, every block 16-byte aligned) so that all loops have compile-time bounds and
// every array lives in registers on the device.  padded_index() maps the flat order of include/mse.h to it.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MSE_PPO_HD __host__ __device__ __forceinline__
#else
#define MSE_PPO_HD inline
#endif

namespace mseppo {

constexpr int kH = 32;
constexpr float kMaskedLogit = -1e8f; // sb3_contrib MaskableCategorical / mse_policy_forward

struct Params {
    float clip_range, ent_coef, vf_coef;
    int normalize_advantage;
    float clip_range_vf; // trailing, so Params{clip, ent, vf, norm} leaves it 0 = off; read by value_head_terms_clipped only
};

// ---- GAE ------------------------------------------------------------------------------------------------------------
// SB3's loop for env column `i` of step-major [K, N] arrays (stride n).  g = float(gamma), gl = float(gamma * lambda)
// (SB3 multiplies the two Python floats first).  Operation order is SB3's:
//   delta = r + g * next_v * nnt - v            ((r + ((g * next_v) * nnt)) - v)
//   gae   = delta + gl * nnt * gae              (delta + ((gl * nnt) * gae))
// Compiled with -ffp-contract=off, so nothing here fuses and the result equals numpy's float32 evaluation bit for bit.
MSE_PPO_HD void gae_column(int k_steps, long long n, long long i, const float *rewards, const float *values,
                           const uint8_t *episode_starts, const float *last_values, const uint8_t *last_dones, float g,
                           float gl, float *adv_out, float *ret_out)
{
    float gae = 0.0f;
    float next_v = last_values[i];
    float nnt = 1.0f - (float)(last_dones[i] != 0 ? 1 : 0);
    for (int k = k_steps - 1; k >= 0; --k) {
        const long long at = (long long)k * n + i;
        const float v = values[at];
        const float t1 = g * next_v;
        const float t2 = t1 * nnt;
        const float t3 = rewards[at] + t2;
        const float delta = t3 - v;
        const float u1 = gl * nnt;
        const float u2 = u1 * gae;
        gae = delta + u2;
        adv_out[at] = gae;
        ret_out[at] = gae + v;
        next_v = v;
        nnt = 1.0f - (float)(episode_starts[at] != 0 ? 1 : 0);
    }
}

// ---- weight layouts -------------------------------------------------------------------------------------------------
// flat order of include/mse.h (= SB3's state_dict order)
struct Flat {
    int pi_w1, pi_b1, pi_w2, pi_b2, act_w, act_b, vf_w1, vf_b1, vf_w2, vf_b2, val_w, val_b, total;
};
MSE_PPO_HD Flat flat_layout(int D, int A)
{
    Flat f;
    f.pi_w1 = 0;
    f.pi_b1 = f.pi_w1 + kH * D;
    f.pi_w2 = f.pi_b1 + kH;
    f.pi_b2 = f.pi_w2 + kH * kH;
    f.act_w = f.pi_b2 + kH;
    f.act_b = f.act_w + A * kH;
    f.vf_w1 = f.act_b + A;
    f.vf_b1 = f.vf_w1 + kH * D;
    f.vf_w2 = f.vf_b1 + kH;
    f.vf_b2 = f.vf_w2 + kH * kH;
    f.val_w = f.vf_b2 + kH;
    f.val_b = f.val_w + kH;
    f.total = f.val_b + 1;
    return f;
}

template <int DP, int AP>
struct Padded {
    static_assert(DP % 4 == 0 && AP % 4 == 0 && DP <= 32 && AP <= 32, "padded sizes are multiples of 4, at most 32");
    static constexpr int pi_w1 = 0;
    static constexpr int pi_b1 = pi_w1 + kH * DP;
    static constexpr int pi_w2 = pi_b1 + kH;
    static constexpr int pi_b2 = pi_w2 + kH * kH;
    static constexpr int act_w = pi_b2 + kH;
    static constexpr int act_b = act_w + AP * kH;
    static constexpr int vf_w1 = act_b + AP;
    static constexpr int vf_b1 = vf_w1 + kH * DP;
    static constexpr int vf_w2 = vf_b1 + kH;
    static constexpr int vf_b2 = vf_w2 + kH * kH;
    static constexpr int val_w = vf_b2 + kH;
    static constexpr int val_b = val_w + kH;
    static constexpr int total = val_b + 4;
};

// flat index (0 <= f < flat_layout(D, A).total) -> index in the padded image
template <int DP, int AP>
MSE_PPO_HD int padded_index(int f, int D, int A)
{
    typedef Padded<DP, AP> P;
    const Flat F = flat_layout(D, A);
    if (f < F.pi_b1) return P::pi_w1 + (f / D) * DP + f % D;
    if (f < F.act_w) return P::pi_b1 + (f - F.pi_b1); // pi_b1, pi_w2, pi_b2 are contiguous in both
    if (f < F.act_b) return P::act_w + (f - F.act_w);
    if (f < F.vf_w1) return P::act_b + (f - F.act_b);
    if (f < F.vf_b1) return P::vf_w1 + ((f - F.vf_w1) / D) * DP + (f - F.vf_w1) % D;
    return P::vf_b1 + (f - F.vf_b1); // vf_b1 .. val_b are contiguous in both
}

// ---- which instantiation of the gradient kernel a policy shape gets -----------------------------------------------------
// Four padded shapes (DP, AP) are compiled: Env_1 (13 -> 2) in (16, 4), Env_2 (16 -> 11) in (16, 12), Env_3 (29 -> 22) in
// (32, 24) and the general (32, 32).  mse_ppo_loss_grad and the host shim of tests/test_ppo_math_cpu.py both ask this
// function and dispatch through MSE_PPO_DISPATCH, so the two cannot drift apart (mse_plan.h does the same for rollouts).
enum GradShape { kShape16x4 = 0, kShape16x12 = 1, kShape32x24 = 2, kShape32x32 = 3, kShapeNone = -1 };

MSE_PPO_HD GradShape select_grad_shape(int D, int A) // 1 <= D, A <= 32, else kShapeNone
{
    if (D < 1 || D > 32 || A < 1 || A > 32) return kShapeNone;
    if (D <= 16 && A <= 4) return kShape16x4;
    if (D <= 16 && A <= 12) return kShape16x12;
    if (A <= 24) return kShape32x24;
    return kShape32x32;
}

MSE_PPO_HD void grad_shape_dims(GradShape s, int &dp, int &ap)
{
    dp = (s == kShape16x4 || s == kShape16x12) ? 16 : 32;
    ap = s == kShape16x4 ? 4 : s == kShape16x12 ? 12 : s == kShape32x24 ? 24 : 32;
}

// MSE_PPO_DISPATCH(shape, CALL): expands CALL(DP, AP) for the instantiation `shape` names; nothing for kShapeNone
#define MSE_PPO_DISPATCH(shape, CALL)                          \
    switch (shape) {                                           \
    case ::mseppo::kShape16x4: CALL(16, 4); break;             \
    case ::mseppo::kShape16x12: CALL(16, 12); break;           \
    case ::mseppo::kShape32x24: CALL(32, 24); break;           \
    case ::mseppo::kShape32x32: CALL(32, 32); break;           \
    default: break;                                            \
    }

// ---- the weight image of the matrix-core gradient kernel (mse_ppo_matrix.hip) --------------------------------------------
// Every 32 x 32 weight block is kept as the A operands of v_mfma_f32_32x32x2_f32: lane (half h, m) supplies, at k-step s,
// the element (m, k) with k = mat_row_of(s, h) - the row an accumulator register s holds in half h, so that an accumulator
// tile is the next product's B operand as it stands.  A block is [4 groups][64 lanes][4 slots] floats, k-step s = 4 group +
// slot: one 16-byte read per lane and group.  Forward blocks have m = output unit, k = input; the blocks the
// back-propagation reads are the transposes (m = input, k = output).  Rows and columns a shape does not have stay zero.
// After the eight blocks come the vectors in natural order, 32 floats each: pi_b1, pi_b2, act_b, vf_b1, vf_b2, val_w, then
// val_b.  The image does not depend on a padded shape.
constexpr int kMatBlockFloats = 32 * 32;
enum MatBlock { kMatPiW1 = 0, kMatPiW2, kMatActW, kMatPiW2T, kMatActWT, kMatVfW1, kMatVfW2, kMatVfW2T, kMatBlocks };
constexpr int kMatPiB1 = kMatBlocks * kMatBlockFloats;
constexpr int kMatPiB2 = kMatPiB1 + 32;
constexpr int kMatActB = kMatPiB2 + 32;
constexpr int kMatVfB1 = kMatActB + 32;
constexpr int kMatVfB2 = kMatVfB1 + 32;
constexpr int kMatValW = kMatVfB2 + 32;
constexpr int kMatValB = kMatValW + 32;
constexpr int kMatTotal = kMatValB + 4;

MSE_PPO_HD int mat_row_of(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; } // = msep::row_of
// element (m, k) of a block -> its cell in the image
MSE_PPO_HD int mat_cell(int block, int m, int k)
{
    const int h = (k >> 2) & 1, s = (k & 3) + 4 * (k >> 3); // k = mat_row_of(s, h)
    return block * kMatBlockFloats + (s >> 2) * 256 + (32 * h + m) * 4 + (s & 3);
}

// flat index (0 <= f < flat_layout(D, A).total) -> the cell of the image every weight has
MSE_PPO_HD int matrix_index(int f, int D, int A)
{
    const Flat F = flat_layout(D, A);
    if (f < F.pi_b1) return mat_cell(kMatPiW1, f / D, f % D);
    if (f < F.pi_w2) return kMatPiB1 + (f - F.pi_b1);
    if (f < F.pi_b2) return mat_cell(kMatPiW2, (f - F.pi_w2) / kH, (f - F.pi_w2) % kH);
    if (f < F.act_w) return kMatPiB2 + (f - F.pi_b2);
    if (f < F.act_b) return mat_cell(kMatActW, (f - F.act_w) / kH, (f - F.act_w) % kH);
    if (f < F.vf_w1) return kMatActB + (f - F.act_b);
    if (f < F.vf_b1) return mat_cell(kMatVfW1, (f - F.vf_w1) / D, (f - F.vf_w1) % D);
    if (f < F.vf_w2) return kMatVfB1 + (f - F.vf_b1);
    if (f < F.vf_b2) return mat_cell(kMatVfW2, (f - F.vf_w2) / kH, (f - F.vf_w2) % kH);
    if (f < F.val_w) return kMatVfB2 + (f - F.vf_b2);
    if (f < F.val_b) return kMatValW + (f - F.val_w);
    return kMatValB;
}

// ... -> the cell of its transposed copy (pi_w2, act_w, vf_w2: what the back-propagation multiplies by), -1 for the rest
MSE_PPO_HD int matrix_index_transposed(int f, int D, int A)
{
    const Flat F = flat_layout(D, A);
    if (f >= F.pi_w2 && f < F.pi_b2) return mat_cell(kMatPiW2T, (f - F.pi_w2) % kH, (f - F.pi_w2) / kH);
    if (f >= F.act_w && f < F.act_b) return mat_cell(kMatActWT, (f - F.act_w) % kH, (f - F.act_w) / kH);
    if (f >= F.vf_w2 && f < F.vf_b2) return mat_cell(kMatVfW2T, (f - F.vf_w2) % kH, (f - F.vf_w2) / kH);
    return -1;
}

// tanh without branches (a lane-divergent libm call would run every path).  Below 0.625: x (1 + u P(u)), u = x^2, P a
// degree-5 least-squares fit of (tanh(x) / x - 1) / u on Chebyshev nodes (error < 1e-10 in exact arithmetic, 4e-8 as
// evaluated in float32).  Above: 1 - 2 q with q = 1 / (e^(2|x|) + 1) <= 0.223, so q's few ulp of relative error stay
// below 1e-7 absolute (6e-8 measured on the host).  The device uses the hardware exp2 and reciprocal (1 ulp each).
MSE_PPO_HD float ppo_tanh(float x)
{
    const float ax = fabsf(x);
    const float u = x * x;
    float poly = fmaf(u, 0.002142803743481636f, -0.008177093230187893f);
    poly = fmaf(u, poly, 0.021700501441955566f);
    poly = fmaf(u, poly, -0.05394670367240906f);
    poly = fmaf(u, poly, 0.1333320587873459f);
    poly = fmaf(u, poly, -0.3333333134651184f);
    poly = fmaf(u * ax, poly, ax);
    // z = 2 log2(e) |x| as z + zl: the product's rounding error (up to 2^-24 z) would otherwise reach e^(2|x|) whole
    const float c_hi = 2.8853900432586670f, c_lo = 3.851925e-8f; // 2 log2(e) = c_hi + c_lo
    const float ac = fminf(ax, 20.0f);                           // tanh(20) rounds to 1
    const float z = ac * c_hi;
    const float zl = fmaf(ac, c_lo, fmaf(ac, c_hi, -z)) * 0.6931471805599453f;
#if defined(__HIP_DEVICE_COMPILE__)
    const float e = __builtin_amdgcn_exp2f(z);
    const float q = __builtin_amdgcn_rcpf(fmaf(e, zl, e) + 1.0f);
#else
    const float e = exp2f(z);
    const float q = 1.0f / (fmaf(e, zl, e) + 1.0f);
#endif
    const float big = fmaf(-2.0f, q, 1.0f);
    return copysignf(ax < 0.625f ? poly : big, x);
}

// ---- the 2 x 32 tanh MLP ------------------------------------------------------------------------------------------------
template <int DP>
MSE_PPO_HD void hidden_forward(const float *w1, const float *b1, const float *w2, const float *b2, const float (&x)[DP],
                               float (&h1)[kH], float (&h2)[kH])
{
#pragma unroll
    for (int o = 0; o < kH; ++o) {
        float acc = b1[o];
#pragma unroll
        for (int i = 0; i < DP; ++i) acc = fmaf(w1[o * DP + i], x[i], acc);
        h1[o] = ppo_tanh(acc);
    }
#pragma unroll
    for (int o = 0; o < kH; ++o) {
        float acc = b2[o];
#pragma unroll
        for (int i = 0; i < kH; ++i) acc = fmaf(w2[o * kH + i], h1[i], acc);
        h2[o] = ppo_tanh(acc);
    }
}

template <int NP>
MSE_PPO_HD void head_forward(const float *w, const float *b, const float (&h2)[kH], float (&out)[NP])
{
#pragma unroll
    for (int a = 0; a < NP; ++a) {
        float acc = b[a];
#pragma unroll
        for (int i = 0; i < kH; ++i) acc = fmaf(w[a * kH + i], h2[i], acc);
        out[a] = acc;
    }
}

// delta of the layer below a linear map: dz[i] = (sum_o w[o][i] d[o]) (1 - h[i]^2)
template <int NP>
MSE_PPO_HD void backprop(const float *w, const float (&d)[NP], const float (&h)[kH], float (&dz)[kH])
{
    float dh[kH];
#pragma unroll
    for (int i = 0; i < kH; ++i) dh[i] = 0.0f;
#pragma unroll
    for (int o = 0; o < NP; ++o) {
#pragma unroll
        for (int i = 0; i < kH; ++i) dh[i] = fmaf(w[o * kH + i], d[o], dh[i]);
    }
#pragma unroll
    for (int i = 0; i < kH; ++i) dz[i] = dh[i] * fmaf(-h[i], h[i], 1.0f);
}

// ---- the heads: loss terms of one row and the gradient w.r.t. the head's outputs -----------------------------------------
struct PolicyTerms {
    float surrogate; // -min(adv ratio, adv clamp(ratio))
    float entropy;   // -sum over legal actions of p log p
    float kl;        // (ratio - 1) - log ratio
    float clipped;   // |ratio - 1| > clip_range
    float logp;      // log-probability of the action taken
};

// logit[a] (a < A real, the rest padding) -> terms; on return logit[] holds
//   d/d logit of ( surrogate + ent_coef * (-entropy) ) * inv_b      (0 for illegal actions and for the padding).
// legal: bit a set = action a may be taken.  torch.min splits a tie evenly and clamp passes the gradient on its closed
// range, so the surrogate's derivative w.r.t. the ratio is adv wherever adv ratio <= adv clamp(ratio), else 0.
template <int AP>
MSE_PPO_HD PolicyTerms policy_head_terms(float (&logit)[AP], int A, uint32_t legal, int action, float old_logp, float adv,
                                         const Params &P, float inv_b)
{
    float m = -INFINITY;
#pragma unroll
    for (int a = 0; a < AP; ++a) {
        if (a < A) {
            logit[a] = ((legal >> a) & 1u) ? logit[a] : kMaskedLogit;
            m = fmaxf(m, logit[a]);
        }
    }
    float s = 0.0f;
#pragma unroll
    for (int a = 0; a < AP; ++a)
        if (a < A) s += expf(logit[a] - m);
    const float lse = m + logf(s);
    float p[AP];
    float ent = 0.0f, mass = 0.0f, logp_act = 0.0f;
#pragma unroll
    for (int a = 0; a < AP; ++a) {
        const bool ok = a < A && ((legal >> a) & 1u);
        const float lp = logit[a] - lse;
        p[a] = ok ? expf(lp) : 0.0f;
        logit[a] = ok ? lp : 0.0f; // now the log-probability
        ent -= ok ? p[a] * lp : 0.0f;
        mass += p[a];
        if (a == action) logp_act = a < A ? lp : 0.0f; // (an illegal action keeps its -1e8-based log-probability)
    }
    PolicyTerms t;
    t.logp = logp_act;
    t.entropy = ent;
    const float log_ratio = logp_act - old_logp;
    const float ratio = expf(log_ratio);
    const float clamped = fminf(fmaxf(ratio, 1.0f - P.clip_range), 1.0f + P.clip_range);
    const float s1 = adv * ratio, s2 = adv * clamped;
    t.surrogate = -fminf(s1, s2);
    t.kl = (ratio - 1.0f) - log_ratio;
    t.clipped = fabsf(ratio - 1.0f) > P.clip_range ? 1.0f : 0.0f;
    const float g_logp = s1 <= s2 ? -(adv * ratio) * inv_b : 0.0f;
    const float ge = P.ent_coef * inv_b, rest = mass - ent; // sum over legal a of p (log p + 1)
#pragma unroll
    for (int a = 0; a < AP; ++a) {
        const bool ok = a < A && ((legal >> a) & 1u);
        const float onehot = a == action ? 1.0f : 0.0f;
        const float d = g_logp * (onehot - p[a]) + ge * (p[a] * (logit[a] + 1.0f) - p[a] * rest);
        logit[a] = ok ? d : 0.0f;
    }
    return t;
}

// ---- behaviour cloning: the cross-entropy of a demonstrated action under the same masked softmax -----------------------------
struct BcTerms {
    float ce;       // -log p(action), 0 where the demonstrated action is illegal under the mask
    float entropy;  // -sum over legal actions of p log p
    float hit;      // 1 where the row is usable and the argmax of the masked logits is the demonstrated action
    float unusable; // 1 where the demonstrated action is illegal under the mask
};

// logit[a] (a < A real, the rest padding) -> terms; on return logit[] holds
//   d/d logit of ( ce + ent_coef * (-entropy) ) * inv_b             (0 for illegal actions and for the padding).
// float32, every operation rounded separately; the softmax, lse, p[a], lp[a], entropy, mass and rest are those of
// policy_head_terms.  `action` is clamped into [0, A) first (clamped_action's rule).  usable = bit `action` of legal:
//   ce = usable ? -lp[action] : 0;   g_logp = usable ? -inv_b : 0
//   logit[a] = g_logp (onehot - p[a]) + ent_coef inv_b (p[a] (lp[a] + 1) - p[a] rest)      for legal a
// so a row whose demonstrated action the mask forbids teaches nothing, yet keeps its entropy term.  The argmax is over the
// masked f32 logits, ties to the lowest index: the rule of the policy head's deterministic mode.
template <int AP>
MSE_PPO_HD BcTerms bc_head_terms(float (&logit)[AP], int A, uint32_t legal, int action, const Params &P, float inv_b)
{
    action = action < 0 ? 0 : (action >= A ? A - 1 : action);
    float m = -INFINITY;
    int best = 0;
#pragma unroll
    for (int a = 0; a < AP; ++a) {
        if (a < A) {
            logit[a] = ((legal >> a) & 1u) ? logit[a] : kMaskedLogit;
            best = logit[a] > m ? a : best;
            m = fmaxf(m, logit[a]);
        }
    }
    float s = 0.0f;
#pragma unroll
    for (int a = 0; a < AP; ++a)
        if (a < A) s += expf(logit[a] - m);
    const float lse = m + logf(s);
    float p[AP];
    float ent = 0.0f, mass = 0.0f, logp_act = 0.0f;
#pragma unroll
    for (int a = 0; a < AP; ++a) {
        const bool ok = a < A && ((legal >> a) & 1u);
        const float lp = logit[a] - lse;
        p[a] = ok ? expf(lp) : 0.0f;
        logit[a] = ok ? lp : 0.0f; // now the log-probability
        ent -= ok ? p[a] * lp : 0.0f;
        mass += p[a];
        if (a == action) logp_act = lp;
    }
    const bool usable = ((legal >> action) & 1u) != 0;
    BcTerms t;
    t.ce = usable ? -logp_act : 0.0f;
    t.entropy = ent;
    t.hit = usable && best == action ? 1.0f : 0.0f;
    t.unusable = usable ? 0.0f : 1.0f;
    const float g_logp = usable ? -inv_b : 0.0f;
    const float ge = P.ent_coef * inv_b, rest = mass - ent; // sum over legal a of p (log p + 1)
#pragma unroll
    for (int a = 0; a < AP; ++a) {
        const bool ok = a < A && ((legal >> a) & 1u);
        const float onehot = a == action ? 1.0f : 0.0f;
        const float d = g_logp * (onehot - p[a]) + ge * (p[a] * (logit[a] + 1.0f) - p[a] * rest);
        logit[a] = ok ? d : 0.0f;
    }
    return t;
}

// ---- PPO with an auxiliary imitation term: both heads on one masked softmax ----------------------------------------------------
struct PolicyBcTerms {
    float surrogate, entropy, kl, clipped, logp; // policy_head_terms' five, for the action taken
    float ce;       // -log p(expert), 0 where the label is illegal under the mask
    float hit;      // 1 where the row is usable and the argmax of the masked logits is the label
    float unusable; // 1 where the label is illegal under the mask
};

// logit[a] (a < A real, the rest padding) -> terms; on return logit[] holds
//   d/d logit of ( surrogate + ent_coef * (-entropy) + bc_coef * ce ) * inv_b    (0 for illegal actions and for the padding).
// float32, every operation rounded separately.  The masked softmax (illegal logits at -1e8, then lse, p[a], lp[a], entropy,
// mass, rest) and the PPO terms of `action` (ratio, clamped, surrogate, kl, clipped, g_logp) are policy_head_terms' to the
// letter; `action` arrives clamped, as it does there.  `expert` is the label, clamped into [0, A) here (clamped_action's
// rule); usable = bit `expert` of legal:
//   ce   = usable ? -lp[expert] : 0
//   hit  = usable && argmax(masked f32 logits, ties to the lowest index) == expert        (bc_head_terms' rule)
//   g_bc = usable ? -(bc_coef * inv_b) : 0                                                (the product rounded once, then negated)
//   logit[a] = g_logp (onehot(a == action) - p[a])  +  g_bc (onehot(a == expert) - p[a])
//              +  ent_coef inv_b (p[a] (lp[a] + 1) - p[a] rest)                           for legal a
// The three summands are added left to right.  With bc_coef = 0 the middle one is +-0, so the sum of the first two is the
// first under ==, and every logit[a] and every PPO term equals policy_head_terms' under ==.  A row whose label the mask forbids
// adds 0 to ce and to the gradient and 1 to unusable, and keeps its PPO and entropy terms.
template <int AP>
MSE_PPO_HD PolicyBcTerms policy_bc_head_terms(float (&logit)[AP], int A, uint32_t legal, int action, int expert, float old_logp,
                                              float adv, const Params &P, float bc_coef, float inv_b)
{
    expert = expert < 0 ? 0 : (expert >= A ? A - 1 : expert);
    float m = -INFINITY;
    int best = 0;
#pragma unroll
    for (int a = 0; a < AP; ++a) {
        if (a < A) {
            logit[a] = ((legal >> a) & 1u) ? logit[a] : kMaskedLogit;
            best = logit[a] > m ? a : best;
            m = fmaxf(m, logit[a]);
        }
    }
    float s = 0.0f;
#pragma unroll
    for (int a = 0; a < AP; ++a)
        if (a < A) s += expf(logit[a] - m);
    const float lse = m + logf(s);
    float p[AP];
    float ent = 0.0f, mass = 0.0f, logp_act = 0.0f, logp_exp = 0.0f;
#pragma unroll
    for (int a = 0; a < AP; ++a) {
        const bool ok = a < A && ((legal >> a) & 1u);
        const float lp = logit[a] - lse;
        p[a] = ok ? expf(lp) : 0.0f;
        logit[a] = ok ? lp : 0.0f; // now the log-probability
        ent -= ok ? p[a] * lp : 0.0f;
        mass += p[a];
        if (a == action) logp_act = a < A ? lp : 0.0f; // (an illegal action keeps its -1e8-based log-probability)
        if (a == expert) logp_exp = lp;
    }
    const bool usable = ((legal >> expert) & 1u) != 0;
    PolicyBcTerms t;
    t.logp = logp_act;
    t.entropy = ent;
    const float log_ratio = logp_act - old_logp;
    const float ratio = expf(log_ratio);
    const float clamped = fminf(fmaxf(ratio, 1.0f - P.clip_range), 1.0f + P.clip_range);
    const float s1 = adv * ratio, s2 = adv * clamped;
    t.surrogate = -fminf(s1, s2);
    t.kl = (ratio - 1.0f) - log_ratio;
    t.clipped = fabsf(ratio - 1.0f) > P.clip_range ? 1.0f : 0.0f;
    t.ce = usable ? -logp_exp : 0.0f;
    t.hit = usable && best == expert ? 1.0f : 0.0f;
    t.unusable = usable ? 0.0f : 1.0f;
    const float g_logp = s1 <= s2 ? -(adv * ratio) * inv_b : 0.0f;
    const float g_bc = usable ? -(bc_coef * inv_b) : 0.0f;
    const float ge = P.ent_coef * inv_b, rest = mass - ent; // sum over legal a of p (log p + 1)
#pragma unroll
    for (int a = 0; a < AP; ++a) {
        const bool ok = a < A && ((legal >> a) & 1u);
        const float on_act = a == action ? 1.0f : 0.0f, on_exp = a == expert ? 1.0f : 0.0f;
        const float d = g_logp * (on_act - p[a]) + g_bc * (on_exp - p[a]) + ge * (p[a] * (logit[a] + 1.0f) - p[a] * rest);
        logit[a] = ok ? d : 0.0f;
    }
    return t;
}

// value -> squared error; dv = d/d value of vf_coef * (returns - value)^2 * inv_b
MSE_PPO_HD float value_head_terms(float value, float ret, const Params &P, float inv_b, float &dv)
{
    const float e = value - ret;
    dv = P.vf_coef * 2.0f * e * inv_b;
    return e * e;
}

// SB3's clip_range_vf (PPO.train: values_pred = old_values + clamp(values - old_values, -c, c), then F.mse_loss(returns,
// values_pred)), c = P.clip_range_vf > 0, every operation rounded separately:
//   d = value - old_value;  dc = min(max(d, -c), c);  vp = old_value + dc;  e = vp - returns
// -> e * e, the squared error of the CLIPPED prediction; dv = d/d value of vf_coef * e^2 * inv_b, which is that of
// value_head_terms where the clamp passes the gradient (d == dc: torch.clamp's closed range) and 0 where it clips.
MSE_PPO_HD float value_head_terms_clipped(float value, float old_value, float ret, const Params &P, float inv_b, float &dv)
{
    const float c = P.clip_range_vf;
    const float d = value - old_value;
    const float dc = fminf(fmaxf(d, -c), c);
    const float vp = old_value + dc;
    const float e = vp - ret;
    dv = d == dc ? P.vf_coef * 2.0f * e * inv_b : 0.0f;
    return e * e;
}

// ---- explained variance: SB3's explained_variance(values, returns) = 1 - var(returns - values) / var(returns) -----------
// Population variances over all n rows, NaN when var(returns) is 0 (n = 1, constant returns).  Specified in full, so that the
// kernels (mse_ppo.hip: k_explained_variance_partial, k_explained_variance_finish) and mse_explained_variance_host add the same
// numbers in the same order and agree bit for bit.  All arithmetic is in double, every operation rounded separately:
//   r_i = (double)returns[i],  d_i = (double)returns[i] - (double)values[i]           (formed in double from the f32 inputs)
//   pivots  pr = r_0,  pd = d_0;   a_i = r_i - pr,  b_i = d_i - pd
//   groups  G = ev_groups(n) = min(kEvMaxGroups, ceil(n / 1024)), each of kEvLanes = 256 lanes;  lane t of group g adds, in
//           ascending i, the elements  i = 256 g + t + 256 G k  (k = 0, 1, ..):  four sums  sum a, sum a^2, sum b, sum b^2
//   tree    within a group, for w = 128, 64, .. 1:  lane t < w adds lane t + w's four sums to its own; lane 0 holds partial g
//   finish  the G partials are added in index order g = 0 .. G - 1, starting from 0  ->  Sa, Qa, Sb, Qb
//           var_r = (Qa - Sa * Sa / n) / n,  var_d = (Qb - Sb * Sb / n) / n          (n converted to double)
//           ev = var_r > 0 ? 1 - var_d / var_r : NaN;   the ONE rounding to f32 is the store of (float)ev
// The pivots keep the sums of squares small beside a mean offset; values == returns gives b_i = 0 and exactly 1.
constexpr int kEvLanes = 256;
constexpr int kEvMaxGroups = 256;
constexpr int kEvRowsPerGroup = 1024; // rows per group below the cap: four trips of a lane

MSE_PPO_HD int ev_groups(long long n)
{
    const long long g = (n + kEvRowsPerGroup - 1) / kEvRowsPerGroup;
    return (int)(g > kEvMaxGroups ? kEvMaxGroups : g);
}

// one lane's four sums: acc[0..3] += over i = first, first + stride, .. < n
MSE_PPO_HD void ev_lane_sums(long long n, long long first, long long stride, const float *values, const float *returns, double (&acc)[4])
{
    const double pr = (double)returns[0], pd = (double)returns[0] - (double)values[0];
    for (long long i = first; i < n; i += stride) {
        const double r = (double)returns[i];
        const double a = r - pr;
        const double b = (r - (double)values[i]) - pd;
        acc[0] += a;
        acc[1] += a * a;
        acc[2] += b;
        acc[3] += b * b;
    }
}

// sums[0..3] = Sa, Qa, Sb, Qb -> the explained variance in double
MSE_PPO_HD double ev_from_sums(const double (&sums)[4], long long n)
{
    const double dn = (double)n;
    const double var_r = (sums[1] - sums[0] * sums[0] / dn) / dn;
    const double var_d = (sums[3] - sums[2] * sums[2] / dn) / dn;
    return var_r > 0.0 ? 1.0 - var_d / var_r : (double)NAN;
}

MSE_PPO_HD float normalized_advantage(float a, float mean, float std) { return (a - mean) / (std + 1e-8f); }

// ---- the minibatch shuffle: a counter-based permutation of [0, total) ------------------------------------------------------
// perm(seed, epoch, total, i) is a function of its four arguments alone (no generator, no state shared between elements), so
// the device fills an epoch's index array with one lane per element and the host replays any element of any epoch
// (mse_ppo_shuffle / mse_ppo_shuffle_host, tests/ppo_shuffle_reference.py restates what follows in numpy).  It is a keyed
// Feistel network on b bits with cycle walking.  All arithmetic is on uint32 and wraps; ^ is xor, >> a logical shift.
//
//   mix32(h):   h ^= h >> 16;  h *= 0x85EBCA6B;  h ^= h >> 13;  h *= 0xC2B2AE35;  h ^= h >> 16      (murmur3's finaliser)
//
//   key (shuffle_key; the only place the 64-bit seed and epoch are read):
//     h = 0x9E3779B9
//     for w in  seed & 0xFFFFFFFF,  seed >> 32,  epoch & 0xFFFFFFFF,  epoch >> 32   (in this order):
//         h = mix32((h ^ w) + 0x9E3779B9)
//     k[r] = mix32(h ^ ((r + 1) * 0x85EBCA77))                 for the six rounds r = 0 .. 5
//   Every absorbing step is a bijection of h for a fixed w and of w for a fixed h, so two seeds that differ in either half
//   (or two epochs) never share h, whatever the other words are.
//
//   split:  b = max(2, ceil(log2 total)) = max(2, number of significant bits of total - 1),  2 <= b <= 31;
//           the LOW half has lo_bits = b / 2 (rounded down) bits, the HIGH half hi_bits = b - lo_bits (the larger when b is odd)
//
//   cipher E on a b-bit value x:   hi = x >> lo_bits;  lo = x & (2^lo_bits - 1)
//     for r = 0 .. 5:   r even:  hi ^= mix32(lo ^ k[r]) & (2^hi_bits - 1)
//                       r odd:   lo ^= mix32(hi ^ k[r]) & (2^lo_bits - 1)
//     E(x) = (hi << lo_bits) | lo
//   Each round xors one half with a function of the other, so E is a bijection of [0, 2^b) for every key.
//
//   shuffle_index(key, total, i):   x = E(i);  while x >= total: x = E(x);  return x
//   Cycle walking: following i's cycle of E until it re-enters [0, total) is a bijection of [0, total).  2^b < 2 total for
//   total >= 2 (2^b = 4 for total = 1), so fewer than two applications of E are expected per element.
constexpr int kShuffleRounds = 6;

struct ShuffleKey {
    uint32_t k[kShuffleRounds];
};

MSE_PPO_HD uint32_t mix32(uint32_t h)
{
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}

MSE_PPO_HD ShuffleKey shuffle_key(uint64_t seed, uint64_t epoch)
{
    const uint32_t words[4] = {(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)epoch, (uint32_t)(epoch >> 32)};
    uint32_t h = 0x9E3779B9u;
    for (int i = 0; i < 4; ++i) h = mix32((h ^ words[i]) + 0x9E3779B9u);
    ShuffleKey key;
    for (int r = 0; r < kShuffleRounds; ++r) key.k[r] = mix32(h ^ ((uint32_t)(r + 1) * 0x85EBCA77u));
    return key;
}

// b for `total` in 1 .. 2^31 (given as uint32)
MSE_PPO_HD int shuffle_bits(uint32_t total)
{
    int b = 0;
    for (uint32_t v = total - 1u; v != 0u; v >>= 1) ++b; // significant bits of total - 1 (a loop: no builtin on the host)
    return b < 2 ? 2 : b;
}

MSE_PPO_HD uint32_t shuffle_index(const ShuffleKey &key, uint32_t total, int bits, uint32_t i) // bits = shuffle_bits(total)
{
    const int lo_bits = bits >> 1, hi_bits = bits - lo_bits;
    const uint32_t lo_mask = (1u << lo_bits) - 1u, hi_mask = (1u << hi_bits) - 1u;
    uint32_t x = i;
    do {
        uint32_t hi = x >> lo_bits, lo = x & lo_mask;
#pragma unroll
        for (int r = 0; r < kShuffleRounds; r += 2) {
            hi ^= mix32(lo ^ key.k[r]) & hi_mask;
            lo ^= mix32(hi ^ key.k[r + 1]) & lo_mask;
        }
        x = (hi << lo_bits) | lo;
    } while (x >= total);
    return x;
}

} // namespace mseppo
