// mse_rollout_modular_body.inc -- the statements of k_rollout_modular's body (mse_lib.hip), included once per __global__ entry:
// k_rollout_modular (LABEL = false) and k_rollout_modular_labelled (LABEL = true), whose further arguments must stay out of
// k_rollout_modular's.  Text and not a function for the reason mse_ppo_grad_body.inc gives.  The including function provides
// the template parameters NOISE and TILES, the constant LABEL, the kernel's arguments and `mix_seed`, `expert_threshold`,
// `labels` (mse_modular_label_buffers; never read with LABEL = false).  Frame: mse_plain_frame.inc.
    using L = PolLayout<3, TILES>; // k_rollout_model's tile: wide enough for every row this kernel stages
    constexpr int ENVS = L::ENVS, NR_SORT = msep::regs_for_actions(2), NR_PRESS = msep::regs_for_actions(11);
    constexpr int kWeightBytes = L::weight_bytes * 2; // [sorting agent image][pressing agent image]
#define MSE_PLAIN_FRAME_PART 1
#include "mse_plain_frame.inc"
    msep_copy_image(lw, sort_blob, true, tid, blockDim.x);
    msep_copy_image(lw + msep::kLdsFloats, press_blob, true, tid, blockDim.x);
#define MSE_PLAIN_FRAME_PART 2
#include "mse_plain_frame.inc"
#define MSE_PLAIN_FRAME_PART 3
#include "mse_plain_frame.inc"
    const msep::lds_f4 wl_sort = (msep::lds_f4)(__attribute__((address_space(3))) float *)lw;
    const msep::lds_f4 wl_press = (msep::lds_f4)(__attribute__((address_space(3))) float *)(lw + msep::kLdsFloats);
    const bool agent_masked = (flags & MSE_MODEL_PRESS_AGENT_MASKED) != 0;
    const bool sort_det = (flags & MSE_MODULAR_SORT_DETERMINISTIC) != 0;
    const bool press_det = (flags & MSE_MODULAR_PRESS_DETERMINISTIC) != 0;
    const uint32_t step_flags = flags & MSE_STEP_CHECK_OVERFLOW; // the agents' actions are applied unsanitised
    // policy stream keys of the env(s) this lane serves as an MFMA column (k_rollout_policy), one pair per agent
    const int h = lane >> 5, col = lane & 31;
    const uint64_t g0 = (uint64_t)(P.index_offset + wave_row0 + col), g1 = g0 + 32u;
    const uint32_t skey0 = mse_policy_key(sort_seed, g0), skey1 = mse_policy_key(sort_seed, g1);
    const uint32_t pkey0 = mse_policy_key(press_seed, g0), pkey1 = mse_policy_key(press_seed, g1);
    int kcur[4]; // container purities of the current state (the sorting view needs them)
    container_purity_k(e, kcur);

    float *ltile = reinterpret_cast<float *>(lwave);
    const uint32_t lrow_sort = lds_row_address(ltile + src_lane * 13);
    const uint32_t lrow_press = lds_row_address(ltile + src_lane * 16);
    const uint32_t lrow_mask = lds_row_address(lwave + src_lane * 11);
    int last_done = 0;
    for (int s = 0; s < k_steps; ++s) {
        const long long srow = (long long)s * P.n + wave_row0;
        const uint64_t t = policy_t0 + (uint64_t)s;
        // ---- the agents' views: get_sort_obs() / get_press_obs() one flow update ahead (a copy takes the update)
        float so[32], po[32];
#pragma unroll
        for (int j = 0; j < 32; ++j) so[j] = po[j] = 0.0f;
        {
            Env ec = e;
            update_environment<false>(ec, P);
            sort_obs<false>(ec, P, tb, kcur, so);
            press_obs<false>(ec, P, tb, po);
        }
        // press_action_masks() of the state the decision is taken in (the flow update does not change it)
        const uint32_t pbits = press_mask_bits(e, P);
        // the rows the decisions are taken from
        if (out.sort_obs != nullptr) wave_store_rows_f32<13, ENVS>(ltile, lrow_sort, so, out.sort_obs + srow * 13, n_valid, lane);
        if (out.press_obs != nullptr) wave_store_rows_f32<16, ENVS>(ltile, lrow_press, po, out.press_obs + srow * 16, n_valid, lane);
        if (out.press_masks != nullptr) wave_store_rows_mask<11, ENVS>(lwave, lrow_mask, pbits, out.press_masks + srow * 11, n_valid, lane);
        if (live && out.episode_starts != nullptr)
            __builtin_nontemporal_store((uint8_t)(e.step == 0 ? 1 : 0), &out.episode_starts[(long long)s * P.n + i]);
        // ---- sorting agent: 13 -> 2, every action legal
        int sm;
        float s_logp, s_value;
        {
            float sx[2][16];
            operands_of(so, sx);
            const uint32_t legal[2] = {legal_of(0x3u, h), legal_of(0x3u, h)};
            const uint32_t words[2] = {mse_policy_word(skey0, t), mse_policy_word(skey1, t)};
            msep::TileOut p[2];
            msep::policy_tiles<NR_SORT, true, TILES>(wl_sort, lane, sx, 2, legal, sort_det, words, nullptr, p);
            sm = tile_pick<TILES>(h, p[0].action, p[1].action);
            s_logp = tile_pick<TILES>(h, p[0].logp, p[1].logp);
            s_value = tile_pick<TILES>(h, p[0].value, p[1].value);
        }
        // ---- pressing agent: 16 -> 11, over press_action_masks() when it is maskable and masking is on
        int pa;
        float p_logp, p_value;
        {
            float px[2][16];
            operands_of(po, px);
            uint32_t pb0, pb1;
            msep::both_halves_u32(agent_masked ? pbits : 0x7FFu, pb0, pb1);
            const uint32_t legal[2] = {legal_of(pb0, h), legal_of(pb1, h)};
            const uint32_t words[2] = {mse_policy_word(pkey0, t), mse_policy_word(pkey1, t)};
            msep::TileOut p[2];
            msep::policy_tiles<NR_PRESS, true, TILES>(wl_press, lane, px, 11, legal, press_det, words, nullptr, p);
            pa = tile_pick<TILES>(h, p[0].action, p[1].action);
            p_logp = tile_pick<TILES>(h, p[0].logp, p[1].logp);
            p_value = tile_pick<TILES>(h, p[0].value, p[1].value);
        }
        int a = sm * 11 + pa;
        [[maybe_unused]] int label = 0;
        [[maybe_unused]] bool expert = false;
        if constexpr (LABEL) {
            // ---- the expert: what mse_rule_actions returns for the state the rows show (k_rollout_demo's label; no stream
            // is read), taken here, after both networks, just before it is needed; and who steps - one decision of
            // mse_demo_mix.h per env and step covers both halves of the flat action.  The mixture's key is the lane's own
            // env's (k_rollout_demo)
            label = rule_based_action<3>(e, Stage<false>::rule_mode(e.st_in, tb));
            const uint32_t mix_key = mse_policy_key(mix_seed, (uint64_t)(P.index_offset + i));
            expert = mse_demo_expert_steps(mix_key, t, expert_threshold);
            a = expert ? label : a;
        }
        // ---- the transition under that action, auto-reset on termination
        float o[32];
        // LABEL: the step reads bale_standard_size through a per-step opaque copy, so that what the compiler derives from it
        // for a branch no step takes (press_bale's fp64 quotient of a count >= 2^24) is formed there and not held in two
        // registers across the loop, where the labelled entry would have to spill it (DESIGN.md 4.19)
        [[maybe_unused]] Params Pstep;
        if constexpr (LABEL) {
            Pstep = P;
            asm volatile("" : "+s"(Pstep.balesize));
        }
        StepResult r = env_step<3, NOISE, false>(e, mse_first_if<LABEL>(Pstep, P), tb, a, -1, step_flags, bales, kcur, o);
        if (__builtin_expect(r.done != 0, 0)) auto_reset_env(e, P, tb, bales, kcur);
        last_done = r.done;
        if constexpr (LABEL) {
            if (live) {
                const long long at = (long long)s * P.n + i;
                if (labels.sort_expert_actions != nullptr) __builtin_nontemporal_store(label / 11, &labels.sort_expert_actions[at]);
                if (labels.press_expert_actions != nullptr) __builtin_nontemporal_store(label % 11, &labels.press_expert_actions[at]);
                if (labels.stepped_actions != nullptr) __builtin_nontemporal_store(a, &labels.stepped_actions[at]);
                if (labels.expert_stepped != nullptr) __builtin_nontemporal_store((uint8_t)(expert ? 1 : 0), &labels.expert_stepped[at]);
            }
        }
        if (live) {
            const long long at = (long long)s * P.n + i;
            if (out.sort_actions != nullptr) __builtin_nontemporal_store(sm, &out.sort_actions[at]);
            if (out.press_actions != nullptr) __builtin_nontemporal_store(pa, &out.press_actions[at]);
            if (out.sort_log_probs != nullptr) __builtin_nontemporal_store(s_logp, &out.sort_log_probs[at]);
            if (out.press_log_probs != nullptr) __builtin_nontemporal_store(p_logp, &out.press_log_probs[at]);
            if (out.sort_values != nullptr) __builtin_nontemporal_store(s_value, &out.sort_values[at]);
            if (out.press_values != nullptr) __builtin_nontemporal_store(p_value, &out.press_values[at]);
            if (out.rewards != nullptr) __builtin_nontemporal_store((float)r.reward, &out.rewards[at]);
            if (out.rewards_sort != nullptr) __builtin_nontemporal_store((float)r.r_sort, &out.rewards_sort[at]);
            if (out.rewards_press != nullptr) __builtin_nontemporal_store((float)r.r_press, &out.rewards_press[at]);
        }
    }
    // the bootstrap values of the state the rollout ends in: each critic alone on its preview of that state
    if (out.sort_last_values != nullptr || out.press_last_values != nullptr) {
        float so[32], po[32];
#pragma unroll
        for (int j = 0; j < 32; ++j) so[j] = po[j] = 0.0f;
        {
            Env ec = e;
            update_environment<false>(ec, P);
            sort_obs<false>(ec, P, tb, kcur, so);
            press_obs<false>(ec, P, tb, po);
        }
        float x[2][16], v[2];
        if (out.sort_last_values != nullptr) {
            operands_of(so, x);
            msep::value_tiles<true, TILES>(wl_sort, lane, x, v);
            if (live) out.sort_last_values[i] = tile_pick<TILES>(h, v[0], v[1]);
        }
        if (out.press_last_values != nullptr) {
            operands_of(po, x);
            msep::value_tiles<true, TILES>(wl_press, lane, x, v);
            if (live) out.press_last_values[i] = tile_pick<TILES>(h, v[0], v[1]);
        }
    }
    if (live && out.last_dones != nullptr) out.last_dones[i] = (uint8_t)last_done;
    if (live) store_env<3, NOISE>(e, planes, P, i, false);
#define MSE_PLAIN_FRAME_PART 4
#include "mse_plain_frame.inc"
