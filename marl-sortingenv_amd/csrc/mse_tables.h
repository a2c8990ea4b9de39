// mse_tables.h -- the config compiler: mse_config -> the kernel arguments (Params, mse_params.h) and the lookup-table
// image the kernels stage in LDS, as plain host C++.  No HIP here, so that
// tests/test_config_tables_cpu.py can compile this header on the host and compare every field and every word with
// tests/config_tables_reference.py.
//
// Bit-for-bit parity with the reference rests on these tables: every quotient of small integers the step would
// evaluate in fp64 is a lookup, and each entry is the reference's own expression evaluated here for each possible
// integer argument (citations = path:line in the reference checkout).  Compile with -ffp-contract=off: numpy rounds
// every operation separately.
//
// The image, in 4-byte words (Params::off_*):
//   lvl     f32[capacity + 1]       clip(float(L / capacity), 0, 1)
//   pdiff   f32[4][kPdiffStride]    clip(float(round(k / 100 - threshold[m], 2)), -1, 1); [101] = an empty container
//   timer0  f32[press_time[0] + 1]  clip(float(t / press_time), 0, 1); timer1 likewise
//   tanh    f64[401]                sorting reward by the sum of the four purity hundredths (8-byte aligned)
//   eff     f64[balesize / 2 + 1]   bale size efficiency by the distance from the standard size
//   acc     f64[3][4]               clip(baseline [+ boost], 0, 1) for sorting mode 0, mode 1, any other mode
//   bonus   f64[4]                  quality peaks - bale_efficiency_factor
//   pat     u32[3][kPatStride]      per-stage-id records (16-byte aligned)
//   ptime   u32[2], qi_down u32[4]
//   cst     f64[CST_COUNT]          config values the step reads as they are
//   jump    u64[kJumpBits][4]       the LCG map of 2^j steps (16-byte aligned; the one-lane rollout copies [0, jump))
//   back    u64[kRingBackSteps][4]  the LCG map of -d steps
//   gprop   f32[256], gfrac f32[256]  general generator mode only
// padded to a multiple of 4 words (copied to LDS in 16-byte pieces).
#pragma once

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "mse.h"
#include "mse_exact.h"
#include "mse_params.h"
#include "mse_plan.h"

namespace mse {

struct CompiledConfig {
    Params P;
    std::vector<uint32_t> image; // the table image, P.table_words words
    bool literal;                // evaluate every Generator.choice draw in literal fp64
    bool noise_on;
};

// The range checks a config passes before anything else looks at it; MSE_OK, or the status with its message in `why`.
inline int config_in_range(const mse_config &c, const char *&why)
{
    why = nullptr;
    if (c.env_kind < MSE_ENV_SORT || c.env_kind > MSE_ENV_MONO) {
        why = "env_kind must be 1 (sort), 2 (press) or 3 (mono)";
        return MSE_ERR_INVALID_ARGUMENT;
    }
    if (c.max_steps < 1 || c.max_steps > 65535) why = "max_steps must be in [1, 65535]";
    else if (c.input_batch_size < 1 || c.input_batch_size > 255) why = "input_batch_size must be in [1, 255]";
    else if (c.press_time[0] < 1 || c.press_time[0] > 255 || c.press_time[1] < 1 || c.press_time[1] > 255)
        why = "press_times must be in [1, 255]";
    else if (c.bale_standard_size < 1 || c.container_capacity < 1 || c.stage_capacity < 1)
        why = "bale_standard_size / container_capacity / stage_capacity must be positive";
    else if (!(c.noise >= 0.0)) why = "noise must be >= 0";
    return why != nullptr ? MSE_ERR_UNSUPPORTED_CONFIG : MSE_OK;
}

// ---- roundings and clips of the reference ---------------------------------------------------------------------------
inline double host_round2(double x) { return std::nearbyint(x * 100.0) / 100.0; } // round(np.float64, 2)
// Python's round(float, 2): correctly rounded on the exact binary value, ties to even (glibc's printf rounds the same
// way) - what the reference computes where the operand is a plain Python float read from config.yml
inline double host_round2_py(double x)
{
    char buf[64];
    std::snprintf(buf, sizeof buf, "%.2f", x);
    return std::strtod(buf, nullptr);
}
inline float host_clip_f(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); } // np.clip on f32
inline double clip01(double v) { return v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v); }                   // np.clip(v, 0, 1)
inline uint32_t f32_bits(float v)
{
    uint32_t u;
    std::memcpy(&u, &v, 4);
    return u;
}

// ---- the 128-bit LCG of PCG64 as an affine map ----------------------------------------------------------------------
// Any number of steps of s' = M s + inc, forward or back, is s -> a s + g inc (mod 2^128): n steps forward have
// a = M^n and g = 1 + M + ... + M^(n-1).  The device applies a map in two 128-bit multiplies (pcg_affine).
typedef unsigned __int128 u128;
struct LcgMap {
    u128 a, g; // in memory A_lo A_hi G_lo G_hi as u64: the order of the table entries and of Params::ring_fwd
};
static_assert(sizeof(LcgMap) == 4 * sizeof(uint64_t), "LcgMap is copied into the image and into Params::ring_fwd");
constexpr LcgMap kLcgStep = {(((u128)0x2360ED051FC65DA4ull) << 64) | (u128)0x4385DF649FCCF645ull, 1}; // pcg64.h
constexpr LcgMap kLcgIdentity = {1, 0};
// first f, then h
inline LcgMap lcg_compose(const LcgMap &f, const LcgMap &h) { return {h.a * f.a, h.a * f.g + h.g}; }
inline LcgMap lcg_power(const LcgMap &f, int n) // n >= 0 times f
{
    LcgMap r = kLcgIdentity;
    for (int i = 0; i < n; ++i) r = lcg_compose(r, f);
    return r;
}
inline LcgMap lcg_inverse(const LcgMap &f)
{
    u128 inv = f.a; // Newton: x <- x (2 - a x) doubles the correct low bits; a * a = 1 mod 8 (a is odd) gives 3 to start
    for (int it = 0; it < 7; ++it) inv = inv * (2 - f.a * inv);
    return {inv, (u128)0 - inv * f.g};
}

// appends to the table image: any f32 / u32 / f64 / u64 / LcgMap value as its 4-byte words, low word first
struct ImageWriter {
    std::vector<uint32_t> &w;
    int at() const { return (int)w.size(); }
    template <class T>
    void put(const T &v)
    {
        uint32_t words[sizeof(T) / 4];
        std::memcpy(words, &v, sizeof(T));
        w.insert(w.end(), words, words + sizeof(T) / 4);
    }
    void align(unsigned words) // a power of two
    {
        while (w.size() & (words - 1u)) w.push_back(0u);
    }
};

// Everything mse_create derives from a config that passed config_in_range: MSE_OK and `out`, or the refusal's status
// with its message in `why`.
inline int compile_config(const mse_config &c, int64_t n_envs, int64_t index_offset, CompiledConfig &out, std::string &why)
{
    const int cap = c.container_capacity, S = c.bale_standard_size;
    Params &P = out.P;
    std::memset(&P, 0, sizeof(P));
    P.n = n_envs;
    P.n_pad = (n_envs + kBlock - 1) / kBlock * kBlock;
    P.index_offset = index_offset;
    P.env_kind = c.env_kind;
    P.max_steps = c.max_steps;
    P.auto_reset = c.auto_reset ? 1 : 0;
    P.track_bales = c.track_bales ? 1 : 0;
    P.balesize = S;
    P.capacity = cap;
    P.stage_capacity = c.stage_capacity;
    P.batch = c.input_batch_size;
    P.press_time[0] = P.press_time0 = c.press_time[0];
    P.press_time[1] = P.press_time1 = c.press_time[1];
    P.inv_balesize = 1.0f / (float)S;
    for (int q = 0; q <= 100; ++q) { // env_super.py:664-666 with the literal expressions
        const double qd = (double)q / 100.0;
        const int qi = (int)(qd * 100.0);
        if (qi != q) P.qi_down[q >> 5] |= 1u << (q & 31);
        if (qi != q && qi != q - 1) {
            why = "int(q*100) is not q or q-1";
            return MSE_ERR_UNSUPPORTED_CONFIG;
        }
    }
    P.rem_thr_units = (int)std::floor((double)S * c.bale_remainder_threshold);
    P.max_state_reward = c.max_state_reward;
    // state_ratio: the reciprocal form up to the first total level where it differs from the literal division, checked
    // over every total a stepped env can hold (no container above capacity + one batch: the overflow ends the
    // episode); a lane beyond that bound divides
    P.sr_den = (double)(5 * cap);
    P.sr_inv = 1.0 / P.sr_den;
    P.sr_exact_max = ratio_exact_upto(P.sr_den, P.sr_inv, 5 * (cap + 255));

    // per-stage-id records: id 0 = the empty stage after reset, 1 / 2 = the seasonal patterns
    uint32_t pat_rec[3][kPatStride];
    for (int k = 0; k < 3; ++k) {
        uint32_t w = 0;
        int sum = 0;
        for (int m = 0; m < 4; ++m) {
            // utils/input_generator.py:47: int(np.floor(ratio * batchsize))
            const int cnt = k == 0 ? 0 : (int)std::floor(c.pattern_ratio[k - 1][m] * (double)c.input_batch_size);
            w |= (uint32_t)cnt << (8 * m);
            sum += cnt;
        }
        // utils/input_generator.py:49-55: units the floor()s leave over go to random materials - general generator mode
        P.gen_rem[k] = k > 0 ? c.input_batch_size - sum : 0;
        if (P.gen_rem[k] != 0) P.gen_mode = 1;
        P.pat_word[k] = w;
        pat_rec[k][0] = w;
        // env_super.py:456 input_occupancy = round(sum/100, 2); get_sort_obs casts to f32 and clips to [-1,1]
        pat_rec[k][1] = f32_bits(host_clip_f((float)((double)sum / 100.0), -1.0f, 1.0f));
        pat_rec[k][3] = 0;
        double pr[4];
        for (int m = 0; m < 4; ++m) {
            const int cnt = (int)((w >> (8 * m)) & 0xFFu);
            pr[m] = sum > 0 ? (double)cnt / (double)sum : 0.0;                                      // env_super.py:199-210
            pat_rec[k][4 + m] = f32_bits(host_clip_f((float)pr[m], -1.0f, 1.0f));
            pat_rec[k][8 + m] = f32_bits(host_clip_f((float)((double)cnt / (double)c.stage_capacity), 0.0f, 1.0f)); // :351
        }
        pat_rec[k][2] = (pr[0] + pr[2] > pr[1] + pr[3]) ? 0u : 1u;                                  // env_super.py:479-482
    }
    P.pat_word1 = P.pat_word[1];
    P.pat_word2 = P.pat_word[2];
    P.occ_nonempty = f32_bits(host_clip_f((float)((double)c.input_batch_size / 100.0), -1.0f, 1.0f)); // env_super.py:456, :318
    if (!P.gen_mode && (P.pat_word[1] == P.pat_word[2] || P.pat_word[1] == 0 || P.pat_word[2] == 0)) {
        why = "the two seasonal patterns must give distinct, non-empty material counts";
        return MSE_ERR_UNSUPPORTED_CONFIG;
    }
    // fill_ratio thresholds of calculate_press_reward as integer levels (env_super.py:1020-1027)
    P.sev_negative = c.overflow_penalty_severe < 0.0 ? 1 : 0;
    P.mild_negative = c.overflow_penalty_mild < 0.0 ? 1 : 0;
    P.thr_sev = P.thr_mild = cap;
    for (int L = cap; L >= 0; --L) {
        const double fill = (double)L / (double)cap;
        if (fill > 0.95) P.thr_sev = L - 1;
        if (fill > 0.90) P.thr_mild = L - 1;
    }
    double acc_rows[3][4]; // np.clip(acc + 0, 0, 1) for mode 0, mode 1, any other mode (env_super.py:499-509)
    for (int m = 0; m < 4; ++m) {
        P.k_thr[m] = (int)std::nearbyint(c.quality_threshold_r2[m] * 100.0);
        if (P.k_thr[m] < 0 || P.k_thr[m] > 100) {
            why = "quality thresholds must lie in [0, 1]";
            return MSE_ERR_UNSUPPORTED_CONFIG;
        }
        const double plain = clip01(c.baseline_accuracy[m]), boosted = clip01(c.baseline_accuracy[m] + c.boost);
        acc_rows[0][m] = (m == 0 || m == 2) ? boosted : plain;
        acc_rows[1][m] = (m == 1 || m == 3) ? boosted : plain;
        acc_rows[2][m] = plain;
        // the lowest accuracy the belt can have: clip(baseline [+ boost] - noise)
        const double lo = clip01(c.baseline_accuracy[m] - c.noise), hi = clip01(c.baseline_accuracy[m] + c.boost - c.noise);
        P.acc_floor[m] = lo < hi ? lo : hi;
    }

    out.image.clear();
    ImageWriter img{out.image};
    P.off_lvl = img.at(); // env_super.py:339-344,359
    for (int L = 0; L <= cap; ++L) img.put(host_clip_f((float)((double)L / (double)cap), 0.0f, 1.0f));
    P.off_pdiff = img.at(); // env_super.py:212-227, 771-791, 325
    for (int m = 0; m < 4; ++m) {
        for (int k = 0; k < kPdiffStride; ++k) {
            // a container's purity is an np.float64 quotient (numpy's round); an EMPTY container's is the threshold, a
            // Python float, and so is its difference (Python's round): env_super.py:212-227, 786-789
            const double diff = k <= 100 ? host_round2((double)k / 100.0 - c.quality_threshold[m])
                                         : host_round2_py(c.quality_threshold_r2[m] - c.quality_threshold[m]);
            img.put(host_clip_f((float)diff, -1.0f, 1.0f));
        }
    }
    P.off_timer0 = img.at(); // env_super.py:354-356
    for (int t = 0; t <= c.press_time[0]; ++t) img.put(host_clip_f((float)((double)t / (double)c.press_time[0]), 0.0f, 1.0f));
    P.off_timer1 = img.at();
    for (int t = 0; t <= c.press_time[1]; ++t) img.put(host_clip_f((float)((double)t / (double)c.press_time[1]), 0.0f, 1.0f));
    img.align(2); // 8-byte alignment of the f64 tables
    P.off_tanh = img.at(); // env_super.py:963-1003 by the sum s of the four purity hundredths
    for (int s = 0; s <= 400; ++s) {
        const long double total = (long double)s / 100.0L - 4.0L * (long double)c.purity_threshold_theta;
        const double state_based = (double)((total / 4.0L) * 2.0L);
        img.put(std::tanh(state_based / c.tanh_temperature));
    }
    P.off_eff = img.at(); // env_super.py:1058-1062
    for (int d = 0; d <= S / 2; ++d) img.put((1.0 - 4.0 * ((double)d / (double)S)) * c.bale_efficiency_factor);
    P.off_acc = img.at();
    for (int r = 0; r < 3; ++r)
        for (int m = 0; m < 4; ++m) img.put(acc_rows[r][m]);
    P.off_bonus = img.at(); // env_super.py:1065-1069
    const double peaks[4] = {0.0, 1.0 / 3.0, 2.0 / 3.0, 1.0}; // env_super.py:1065
    for (int b = 0; b < 4; ++b) img.put(peaks[b] - c.bale_efficiency_factor);
    img.align(4); // 16-byte alignment of the per-stage records (read as float4)
    P.off_pat = img.at();
    for (int k = 0; k < 3; ++k)
        for (int w = 0; w < kPatStride; ++w) img.put(pat_rec[k][w]);
    P.off_ptime = img.at();
    img.put((uint32_t)c.press_time[0]);
    img.put((uint32_t)c.press_time[1]);
    for (int w = 0; w < 4; ++w) img.put(P.qi_down[w]); // bale_quality_int's mask
    P.off_cst = img.at(); // even: every section so far has an even word count after off_tanh
    {
        double cst[CST_COUNT] = {};
        cst[CST_PEN_CAT] = c.overflow_penalty_catastrophic;
        cst[CST_PEN_SEV] = c.overflow_penalty_severe;
        cst[CST_PEN_MILD] = c.overflow_penalty_mild;
        cst[CST_MAX_STATE] = c.max_state_reward;
        cst[CST_OVERFLOW_PEN] = c.overflow_termination_penalty;
        cst[CST_REM_THR] = c.bale_remainder_threshold;
        cst[CST_BOOST] = c.boost;
        cst[CST_NOISE] = c.noise;
        for (int m = 0; m < 4; ++m) cst[CST_BASE_ACC0 + m] = c.baseline_accuracy[m];
        for (int k = 0; k < CST_COUNT; ++k) img.put(cst[k]);
    }
    img.align(4); // the one-lane rollout kernel copies [0, off_jump) in 16-byte pieces
    P.off_jump = img.at(); // jump ahead by 2^j steps (pcg_jump)
    LcgMap f = kLcgStep;
    for (int j = 0; j < kJumpBits; ++j, f = lcg_compose(f, f)) img.put(f);
    P.off_back = img.at(); // even; jump back by d steps (pcg_step_back)
    f = kLcgIdentity;
    for (int d = 0; d < kRingBackSteps; ++d, f = lcg_compose(f, kLcgStep)) img.put(lcg_inverse(f));
    P.off_gprop = P.off_gfrac = 0;
    if (P.gen_mode) { // per-count tables: every batch holds input_batch_size units, so a share is a function of the count
        P.off_gprop = img.at();
        for (int k = 0; k < 256; ++k) img.put(host_clip_f((float)((double)k / (double)c.input_batch_size), -1.0f, 1.0f));
        P.off_gfrac = img.at();
        for (int k = 0; k < 256; ++k) img.put(host_clip_f((float)((double)k / (double)c.stage_capacity), 0.0f, 1.0f));
    }
    img.align(4); // copied to LDS in 16-byte pieces
    P.table_words = img.at();
    if (P.table_words > 16384) {
        why = "container_capacity / bale_standard_size too large for the LDS-resident tables (64 KiB)";
        return MSE_ERR_UNSUPPORTED_CONFIG;
    }

    out.noise_on = c.noise != 0.0;
    // the byte-packed integer draw needs every prefix sum below 128; larger batches draw in literal fp64
    out.literal = c.literal_choice != 0 || c.input_batch_size > 127;
    P.ring_worst = max_draws_per_step(c.baseline_accuracy, c.boost, c.noise, P.pat_word, c.env_kind);
    // the distance between the two halves of the ring's priming (k_rollout_ring)
    const LcgMap fwd = lcg_power(kLcgStep, P.ring_worst);
    std::memcpy(P.ring_fwd, &fwd, sizeof(P.ring_fwd));
    return MSE_OK;
}

} // namespace mse
