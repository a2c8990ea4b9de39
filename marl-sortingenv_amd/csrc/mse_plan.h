// mse_plan.h -- which rollout kernel a launch runs, and the shape it runs in: the selection policy of mse_rollout,
// mse_rollout_policy and mse_rollout_model as plain host C++.  No HIP here: the LDS sizes that depend on
// a kernel's layout (RingLayout, PolRolesLayout, PolLayout in mse_lib.hip) come in as numbers, so that
// tests/test_rollout_plan.py can compile this header on the host and check the table.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "mse.h" // status codes, env kinds

namespace mse {

constexpr size_t kLdsLimitBytes = 160 * 1024; // LDS of one CU, the most one workgroup can ask for
constexpr int kPlanRingMaxPerStep = 31;       // = kRingMaxPerStep (mse_device.h; asserted in mse_lib.hip)
constexpr int64_t kRoundEnvs = 256;           // envs per CU in one round of the multi-role kernels (kPoEnvs)

// The most sort_material draws one step can make with the config: the mis-sorted units of the two stations a mode
// leaves unboosted, at the lowest accuracy the noise allows.  false_m = target - rint(target * acc) grows with target
// (<= the pattern's count) and falls with acc (>= clip(baseline [+ boost] - noise)); modes other than 0 / 1 (no boost)
// exist only for Env_2's externally supplied sorting decision.  pat_word: Params::pat_word, the counts A..D of
// patterns 1 and 2 packed one byte each.
inline int max_draws_per_step(const double baseline[4], double boost, double noise, const uint32_t pat_word[3],
                              int env_kind)
{
    int worst = 0;
    const int n_modes = env_kind == MSE_ENV_PRESS ? 3 : 2;
    for (int k = 1; k <= 2; ++k) {
        for (int mode = 0; mode < n_modes; ++mode) {
            int sum = 0;
            for (int m = 0; m < 4; ++m) {
                const bool boosted = mode == 0 ? (m == 0 || m == 2) : (mode == 1 ? (m == 1 || m == 3) : false);
                double acc = baseline[m] + (boosted ? boost : 0.0) - noise;
                acc = acc < 0.0 ? 0.0 : (acc > 1.0 ? 1.0 : acc);
                const int cnt = (int)((pat_word[k] >> (8 * m)) & 0xFFu);
                sum += cnt - (int)nearbyint((double)cnt * acc);
            }
            worst = sum > worst ? sum : worst;
        }
    }
    return worst;
}

// the batch fits the chip in one round: one 256-env workgroup per CU
inline bool one_round(int64_t n_envs, int cus) { return n_envs <= kRoundEnvs * cus; }

// what an LDS ring needs besides its LDS image: two steps' draws in the ring, the integer draw path, and a build
// whose ring kernels keep the ring at LDS address 0 (no static __shared__, ring_kernels_static_lds_free)
inline bool ring_draws_fit(int worst, bool literal, bool ring_static_lds_free)
{
    return worst <= kPlanRingMaxPerStep && !literal && ring_static_lds_free;
}

// ---- mse_rollout ----------------------------------------------------------------------------------------------------
enum class RolloutKernel { OneLane, TwoRole, Ring }; // k_rollout, k_rollout_po, k_rollout_ring

struct RolloutPlan {
    RolloutKernel kernel;
    int status;      // MSE_OK, or mse_create's refusal of the config with message `why`
    const char *why;
};

// mse_config::rollout_pipeline: 0 = decide by size, 1 = two roles, 2 = one lane per env, 3 = three roles (ring).
// The multi-role kernels serve 256 envs per workgroup, one workgroup per CU (their LDS image is the whole CU's), so
// they pay off exactly while the batch fits the chip in one round: n <= 256 x CUs (65 536 on an MI355X).  Beyond that
// a one-lane-per-env grid already gives every SIMD several waves and wins (measured at 131 072 envs: 16.5 G
// env-steps/s against 15.9) - except while the batch fills most of a SECOND round: same-box at 64 steps per launch,
// three-role kernel against one lane per env: 98 304 envs 17.5 G against 15.5, 131 072 envs 22.9 against 20.5 (two
// full rounds run at the one-round rate; the one-lane grid has only two waves per SIMD there), 196 608 envs 23.1
// against 23.8.  That second-round rule was measured with the three-role kernel only.  ring_lds_bytes: k_rollout_ring's
// LDS image (ring, obs tile, two snapshots, bale ledger, tables).
inline RolloutPlan plan_rollout(int rollout_pipeline, int64_t n_envs, int cus, bool literal, bool gen_mode, int worst,
                                size_t ring_lds_bytes, bool ring_static_lds_free)
{
    const int rp = rollout_pipeline;
    if (gen_mode && (rp == 1 || rp == 3)) // general generator mode: the multi-role kernels carry stage ids, not counts
        return {RolloutKernel::OneLane, MSE_ERR_UNSUPPORTED_CONFIG,
                "rollout_pipeline 1 / 3 need a remainder-free input_batch_size (the one-lane kernels serve the general "
                "generator)"};
    const bool fits = ring_draws_fit(worst, literal, ring_static_lds_free) && ring_lds_bytes <= kLdsLimitBytes;
    if (rp == 3 && !fits)
        return {RolloutKernel::OneLane, MSE_ERR_UNSUPPORTED_CONFIG,
                "rollout_pipeline=3 (ring kernel) needs at most 31 draws per step, the integer draw path and an LDS "
                "image within 160 KiB"};
    const int64_t n_wg = (n_envs + kRoundEnvs - 1) / kRoundEnvs;
    const bool second_round = n_wg > cus + cus / 4 && n_wg <= 2 * (int64_t)cus;
    const bool multi_role = !gen_mode && (rp == 1 || rp == 3 || (rp == 0 && (n_wg <= cus || (second_round && fits))));
    if (!multi_role) return {RolloutKernel::OneLane, MSE_OK, nullptr};
    return {fits && rp != 1 ? RolloutKernel::Ring : RolloutKernel::TwoRole, MSE_OK, nullptr};
}

// ---- mse_rollout_policy / mse_rollout_model -------------------------------------------------------------------------
enum class PolicyKernel { RolesRing, Roles, Plain }; // k_rollout_policy_roles<RING = true / false>, k_rollout_policy

struct PolicyLds {        // bytes, from the kernels' layouts
    size_t roles_ring;    // k_rollout_policy_roles<RING = true>, tables included
    size_t roles_pair;    // k_rollout_policy_roles<RING = false>, tables included
    size_t network;       // one network's LDS image (msep::kLdsFloats)
    size_t tables;        // the config's table image
    size_t wave[2];       // k_rollout_policy's per-wave staging with 1 / 2 tiles (PolLayout::wave_bytes)
};

struct PolicyPlan {
    int status;           // MSE_OK, or MSE_ERR_UNSUPPORTED_CONFIG: the LDS image does not fit
    PolicyKernel kernel;
    size_t lds_bytes;     // the dynamic LDS the kernel asks for
    int tiles, n_waves;   // Plain: 32 x tiles envs per wave, n_waves waves per workgroup
    int64_t workgroups;
};

// k_rollout_policy's shape, which k_rollout_model (f16x3, two networks) shares: eight waves per workgroup, two per
// SIMD.  While 32-env waves leave every CU at most one workgroup's worth (n <= 256 envs x CUs) a wave owns 32 envs - at
// that size 64-env waves would run one per SIMD, at a vector instruction per ~5 cycles; beyond, 64 envs.  The exact-f32
// form only exists in the 64-env shape: below that size four 64-env waves per workgroup, so that every CU gets one.
inline PolicyPlan plan_policy_plain(int64_t n_envs, int cus, bool f16, int n_networks, const PolicyLds &lds)
{
    const bool small = one_round(n_envs, cus);
    const int tiles = f16 && small ? 1 : 2, n_waves = !f16 && small ? 4 : 8;
    const size_t bytes = lds.network * (size_t)n_networks + lds.tables + (size_t)n_waves * lds.wave[tiles - 1];
    const int64_t envs_per_wg = 32LL * tiles * n_waves;
    return {bytes > kLdsLimitBytes ? MSE_ERR_UNSUPPORTED_CONFIG : MSE_OK, PolicyKernel::Plain, bytes, tiles, n_waves,
            (n_envs + envs_per_wg - 1) / envs_per_wg};
}

// mse_rollout_policy: batches that leave a SIMD 64 envs (n <= 256 envs x CUs), f16x3 form, no in-loop sorting policy
// run the kernel in roles (one workgroup of four actor / critic[ / RNG] wave sets per 256 envs).  rollout_pipeline =
// 2 keeps the plain kernel and 1 the form without the RNG waves, which is how the tests hold the three together.
inline PolicyPlan plan_rollout_policy(int rollout_pipeline, int64_t n_envs, int cus, bool f16, bool sort_policy,
                                      int worst, bool literal, bool gen_mode, bool ring_static_lds_free,
                                      const PolicyLds &lds)
{
    if (f16 && !sort_policy && one_round(n_envs, cus) && rollout_pipeline != 2) {
        const int64_t wgs = (n_envs + kRoundEnvs - 1) / kRoundEnvs;
        const bool ring_ok = ring_draws_fit(worst, literal, ring_static_lds_free) && !gen_mode;
        if (ring_ok && lds.roles_ring <= kLdsLimitBytes && rollout_pipeline != 1)
            return {MSE_OK, PolicyKernel::RolesRing, lds.roles_ring, 0, 0, wgs};
        if (lds.roles_pair <= kLdsLimitBytes) return {MSE_OK, PolicyKernel::Roles, lds.roles_pair, 0, 0, wgs};
    }
    return plan_policy_plain(n_envs, cus, f16, sort_policy ? 2 : 1, lds);
}

} // namespace mse
