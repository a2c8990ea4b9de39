// mse_rollout_policy_body.inc -- the statements of k_rollout_policy's body (mse_lib.hip), included once per __global__ entry:
// k_rollout_policy (LABEL = false) and k_rollout_policy_labelled (LABEL = true), whose one more argument must stay out of
// k_rollout_policy's.  Text and not a function for the reason mse_ppo_grad_body.inc gives.  The including function provides
// the template parameters KIND, NOISE, TILES, F16X3, the constants SORTPOL and LABEL, the kernel's arguments and `expert_out`
// (i32[K, N]; never read with LABEL = false).  Frame: mse_plain_frame.inc.
    using L = PolLayout<KIND, TILES>;
    constexpr int D = L::D, A = L::A, NR = msep::regs_for_actions(A), ENVS = L::ENVS;
    constexpr int kWeightBytes = L::weight_bytes * (SORTPOL ? 2 : 1); // [policy image][sorting policy image]
#define MSE_PLAIN_FRAME_PART 1
#include "mse_plain_frame.inc"
    msep_copy_image(lw, weight_blob, F16X3, tid, blockDim.x);
    if (SORTPOL) msep_copy_image(lw + msep::kLdsFloats, sort_weight_blob, F16X3, tid, blockDim.x);
#define MSE_PLAIN_FRAME_PART 2
#include "mse_plain_frame.inc"
    int sm = -1;
    if (KIND == 2 && sort_mode != nullptr) sm = sort_mode[i];
#define MSE_PLAIN_FRAME_PART 3
#include "mse_plain_frame.inc"
    msep::lds_f4 wl = (msep::lds_f4)(__attribute__((address_space(3))) float *)lw;

    // the observation and mask of the current state (what reset / the previous launch left)
    float o[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) o[j] = 0.0f;
    int kcur[4]; // container purities of the current state (the sorting agent's view needs them)
    container_purity_k(e, kcur);
    env_obs<KIND>(e, P, tb, kcur, o);
    uint32_t mbits = action_mask_bits<KIND>(e, P);
    msep::lds_f4 wl_sort = (msep::lds_f4)(__attribute__((address_space(3))) float *)(lw + msep::kLdsFloats);
    // policy stream keys of the env(s) this lane serves as an MFMA column: tile t = envs 32 t .. 32 t + 31 of the wave
    const int h = lane >> 5, col = lane & 31;
    const uint32_t key0 = mse_policy_key(policy_seed, (uint64_t)(P.index_offset + wave_row0 + col));
    const uint32_t key1 = mse_policy_key(policy_seed, (uint64_t)(P.index_offset + wave_row0 + 32 + col));

    const uint32_t lrow_obs = lds_row_address(reinterpret_cast<float *>(lwave) + src_lane * D);
    const uint32_t lrow_mask = lds_row_address(lwave + src_lane * A);
    int last_done = 0;
#ifdef MSE_TIMELINE
    Timeline ptl;
    ptl.start();
#endif
    for (int s = 0; s < k_steps; ++s) {
        __builtin_amdgcn_s_setprio(TILES == 2 ? 3 : 0); // policy phase (see below)
        const long long srow = (long long)s * P.n + wave_row0;
        // the row the action is taken from (MaskableRolloutBuffer: observations, action_masks, episode_starts)
        if (obs_out != nullptr) wave_store_rows_f32<D, ENVS>(reinterpret_cast<float *>(lwave), lrow_obs, o, obs_out + srow * D, n_valid, lane);
        if (mask_out != nullptr) wave_store_rows_mask<A, ENVS>(lwave, lrow_mask, mbits, mask_out + srow * A, n_valid, lane);
        if (live && start_out != nullptr)
            __builtin_nontemporal_store((uint8_t)(e.step == 0 ? 1 : 0), &start_out[(long long)s * P.n + i]);
        if constexpr (LABEL) { // what mse_rule_actions returns for the state the row shows (k_rollout_demo's label); no stream is read
            const int label = rule_based_action<KIND>(e, Stage<false>::rule_mode(e.st_in, tb));
            if (live) __builtin_nontemporal_store(label, &expert_out[(long long)s * P.n + i]);
        }
        MSE_TLB(ptl, 0); // row stores
        // ---- policy
        float x[2][16];
        operands_of(o, x);
        // without masking (plain PPO on the unmasked env) the policy samples from the whole action space and the
        // step sanitises; the recorded mask row is action_masks() either way
        uint32_t mb0, mb1;
        msep::both_halves_u32((flags & MSE_STEP_UNMASKED) ? ((1u << A) - 1u) : mbits, mb0, mb1);
        const uint64_t t = policy_t0 + (uint64_t)s;
        const uint32_t legal[2] = {legal_of(mb0, h), legal_of(mb1, h)};
        const uint32_t words[2] = {mse_policy_word(key0, t), mse_policy_word(key1, t)};
        msep::TileOut p[2];
        msep::policy_tiles<NR, F16X3, TILES>(wl, lane, x, A, legal, deterministic != 0, words, nullptr, p);
        const int a = tile_pick<TILES>(h, p[0].action, p[1].action);
        const float logp = tile_pick<TILES>(h, p[0].logp, p[1].logp), value = tile_pick<TILES>(h, p[0].value, p[1].value);
        MSE_TLB(ptl, 1); // policy forward
        // Phase priorities: the two waves of a SIMD fall into step with each other (both in the policy, both in the
        // dynamics) and then compete for the same pipe; letting one phase win the issue arbitration pulls them apart so
        // that one wave's MFMA chains run under the other's dynamics.  Which phase should win was measured on the box
        // (same-box A/B, 16 steps per launch): 64-env waves +8 % with the policy phase high, 32-env waves +8 % with the
        // dynamics phase high (the other choice +4 ... 6 % each; a static per-wave priority: nothing).
        __builtin_amdgcn_s_setprio(TILES == 2 ? 0 : 3);
        if (SORTPOL) {
            // the sorting agent's decision for the coming step: get_sort_obs() one flow update ahead (a copy steps
            // the flow; env_step will take the same step), through the second network's actor, argmax
            float so[32];
#pragma unroll
            for (int j = 0; j < 32; ++j) so[j] = 0.0f;
            {
                Env ec = e;
                update_environment<false>(ec, P);
                sort_obs<false>(ec, P, tb, kcur, so);
            }
            float sx[2][16];
            operands_of(so, sx);
            int sa[2];
            msep::actor_argmax2_tiles<F16X3, TILES>(wl_sort, lane, sx, sa);
            sm = tile_pick<TILES>(h, sa[0], sa[1]);
        }
        MSE_TLB(ptl, 2); // sorting agent
        // ---- the env transition under that action
        StepResult r = env_step<KIND, NOISE, false>(e, P, tb, a, sm, flags, bales, kcur, o);
        MSE_TLB(ptl, 3); // env transition
        if (__builtin_expect(r.done != 0, 0)) {
            auto_reset_env(e, P, tb, bales, kcur);
            env_obs<KIND>(e, P, tb, kcur, o);
        }
        mbits = action_mask_bits<KIND>(e, P);
        last_done = r.done;
        if (live) {
            const long long at = (long long)s * P.n + i;
            if (actions_out != nullptr) __builtin_nontemporal_store(a, &actions_out[at]);
            if (logp_out != nullptr) __builtin_nontemporal_store(logp, &logp_out[at]);
            if (value_out != nullptr) __builtin_nontemporal_store(value, &value_out[at]);
            if (reward_out != nullptr) __builtin_nontemporal_store((float)r.reward, &reward_out[at]);
        }
        MSE_TLB(ptl, 4); // auto-reset, mask, per-env stores
    }
#ifdef MSE_TIMELINE
    ptl.flush(0);
#endif
    // the bootstrap value of the state the rollout ends in: the critic alone
    if (last_value_out != nullptr) {
        float x[2][16], v[2];
        operands_of(o, x);
        msep::value_tiles<F16X3, TILES>(wl, lane, x, v);
        if (live) last_value_out[i] = tile_pick<TILES>(h, v[0], v[1]);
    }
    if (live && last_done_out != nullptr) last_done_out[i] = (uint8_t)last_done;
    if (live) store_env<KIND, NOISE>(e, planes, P, i, false);
#define MSE_PLAIN_FRAME_PART 4
#include "mse_plain_frame.inc"
