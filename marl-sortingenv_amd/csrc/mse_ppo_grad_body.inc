// mse_ppo_grad_body.inc -- the statements of k_ppo_grad's body (mse_ppo.hip), included once per __global__ entry of the kernel:
// k_ppo_grad (KICK = false) and k_ppo_grad_kick (KICK = true), whose two more arguments must stay out of k_ppo_grad's.  It is
// text and not a function, because no helper form kept k_ppo_grad's instructions (tools/same_isa.py): an inlined body moves the
// kernel's exit and its register allocation.  The including function provides the template parameters DP, AP, VCLIP, the
// constants BC and KICK, the kernel's arguments and `K` (KickArgs; never read with KICK = false).  Likewise k_ppo_grad_shard
// (SHARD = true) with `S` (ShardArgs; never read with SHARD = false): G.batch bounds the local rows, S.global_batch scales the
// per-row terms, the advantage mean and std come from S.moments.
    typedef Padded<DP, AP> PW;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    if (gate_closed(control)) { // grid-uniform
        mark_gate_closed(flat_layout(G.D, G.A).total, slabs);
        return;
    }
    float *wl0 = lds;                     // PW::total floats: the padded weights
    float *strips = lds + PW::total;      // 4 x kStageFloats: one staging strip per wave
    float *misc = strips + 4 * kStageFloats; // kMiscFloats (KICK: kKickMiscFloats)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int D = G.D, A = G.A;
    const Flat F = flat_layout(D, A);
    for (int i = tid; i < PW::total; i += 256) wl0[i] = 0.0f;
    __syncthreads();
    for (int f = tid; f < F.total; f += 256) wl0[padded_index<DP, AP>(f, D, A)] = weights[f];
    if constexpr (SHARD)
        publish_shard_mean_std(G, S, misc, wave, lane);
    else
        publish_adv_mean_std(G, rows, adv, adv_partial, misc, wave, lane);
    __syncthreads();
    const bool normalize = G.n_adv_partial > 0;
    const float mean = misc[0], std = misc[1];
    const float inv_b_all = 1.0f / (float)(SHARD ? S.global_batch : G.batch); // SHARD: G.batch is the local row bound
    const bool critic = (wave & 1) != 0;
    float *strip = strips + wave * kStageFloats;
    LayerAcc L1 = {}, L2 = {}, L3 = {}; // first, second hidden layer, head
    float st0 = 0.0f, st1 = 0.0f, st2 = 0.0f, st3 = 0.0f;
    [[maybe_unused]] float st4 = 0.0f, st5 = 0.0f, st6 = 0.0f; // KICK only
    long long n_tiles = (G.batch + 63) / 64;
    if constexpr (BC) n_tiles = critic && ret == nullptr ? 0 : n_tiles; // wave-uniform: no returns, nothing for the critic
    for (long long tile = (long long)blockIdx.x * 2 + (wave >> 1); tile < n_tiles; tile += (long long)gridDim.x * 2) {
        // the weights are re-read from LDS every tile: an offset the compiler cannot see through keeps it from hoisting
        // ~5 000 wave-uniform values out of the loop into (spilled) scalar registers
        unsigned opaque = 0;
        asm volatile("" : "+v"(opaque));
        const float *wl = static_cast<const float *>(__builtin_assume_aligned(wl0 + 4 * opaque, 16));
        const long long b = tile * 64 + lane;
        const bool valid = b < G.batch;
        const long long row = row_at(rows, valid ? b : 0, G.n_rows);
        const float inv_b = valid ? inv_b_all : 0.0f; // a padding lane contributes zero deltas
        float x[DP];
#pragma unroll
        for (int i = 0; i < DP; ++i) {
            const float v = obs[row * D + (i < D ? i : 0)];
            x[i] = i < D ? v : 0.0f;
        }
        float h1[kH], h2[kH], dz[kH];
        if (!critic) {
            uint32_t legal = 0;
#pragma unroll
            for (int a = 0; a < AP; ++a) {
                const bool ok = a < A && (mask == nullptr || mask[row * A + (a < A ? a : 0)] != 0);
                legal |= (ok ? 1u : 0u) << a;
            }
            float dl[AP];
            if constexpr (KICK) {
                const int action = clamped_action(actions[row], A);
                const float a_raw = adv[row];
                const float a_used = normalize ? normalized_advantage(a_raw, mean, std) : a_raw;
                hidden_forward<DP>(wl + PW::pi_w1, wl + PW::pi_b1, wl + PW::pi_w2, wl + PW::pi_b2, x, h1, h2);
                head_forward<AP>(wl + PW::act_w, wl + PW::act_b, h2, dl);
                const PolicyBcTerms t =
                    policy_bc_head_terms<AP>(dl, A, legal, action, K.expert_actions[row], old_logp[row], a_used, G.P, K.bc_coef, inv_b);
                if (valid) {
                    st0 += t.surrogate;
                    st1 += t.entropy;
                    st2 += t.kl;
                    st3 += t.clipped;
                    st4 += t.ce;
                    st5 += t.hit;
                    st6 += t.unusable;
                }
            } else if constexpr (BC) {
                hidden_forward<DP>(wl + PW::pi_w1, wl + PW::pi_b1, wl + PW::pi_w2, wl + PW::pi_b2, x, h1, h2);
                head_forward<AP>(wl + PW::act_w, wl + PW::act_b, h2, dl);
                const BcTerms t = bc_head_terms<AP>(dl, A, legal, actions[row], G.P, inv_b);
                if (valid) {
                    st0 += t.ce;
                    st1 += t.entropy;
                    st2 += t.hit;
                    st3 += t.unusable;
                }
            } else {
                const int action = clamped_action(actions[row], A);
                const float a_raw = adv[row];
                const float a_used = normalize ? normalized_advantage(a_raw, mean, std) : a_raw;
                hidden_forward<DP>(wl + PW::pi_w1, wl + PW::pi_b1, wl + PW::pi_w2, wl + PW::pi_b2, x, h1, h2);
                head_forward<AP>(wl + PW::act_w, wl + PW::act_b, h2, dl);
                const PolicyTerms t = policy_head_terms<AP>(dl, A, legal, action, old_logp[row], a_used, G.P, inv_b);
                if (valid) {
                    st0 += t.surrogate;
                    st1 += t.entropy;
                    st2 += t.kl;
                    st3 += t.clipped;
                }
            }
            accumulate_layer(strip, lane, dl, h2, L3.w, L3.b);
            backprop<AP>(wl + PW::act_w, dl, h2, dz);
        } else {
            hidden_forward<DP>(wl + PW::vf_w1, wl + PW::vf_b1, wl + PW::vf_w2, wl + PW::vf_b2, x, h1, h2);
            float v[1];
            head_forward<1>(wl + PW::val_w, wl + PW::val_b, h2, v);
            float dv[1];
            float sq;
            if constexpr (VCLIP)
                sq = value_head_terms_clipped(v[0], old_values[row], ret[row], G.P, inv_b, dv[0]);
            else
                sq = value_head_terms(v[0], ret[row], G.P, inv_b, dv[0]);
            if (valid) st0 += sq;
            accumulate_layer(strip, lane, dv, h2, L3.w, L3.b);
            backprop<1>(wl + PW::val_w, dv, h2, dz);
        }
        const float *w2 = wl + (critic ? PW::vf_w2 : PW::pi_w2);
        accumulate_layer(strip, lane, dz, h1, L2.w, L2.b);
        float dz1[kH];
        backprop<kH>(w2, dz, h1, dz1);
        accumulate_layer(strip, lane, dz1, x, L1.w, L1.b);
    }
    // ---- the two waves of a network: slot 1 hands its sums to slot 0 through LDS; fixed order (slot 0 + slot 1) ----
    st0 = wave_sum(st0);
    st1 = wave_sum(st1);
    st2 = wave_sum(st2);
    st3 = wave_sum(st3);
    if constexpr (KICK) {
        st4 = wave_sum(st4);
        st5 = wave_sum(st5);
        st6 = wave_sum(st6);
    }
    __syncthreads(); // every wave is done with its strip
    float *xch = strips + (wave & 1) * (60 * 64);
    if (wave >= 2) {
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            xch[(k)*64 + lane] = L1.w[k];
            xch[(16 + k) * 64 + lane] = L2.w[k];
            xch[(32 + k) * 64 + lane] = L3.w[k];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            xch[(48 + k) * 64 + lane] = L1.b[k];
            xch[(52 + k) * 64 + lane] = L2.b[k];
            xch[(56 + k) * 64 + lane] = L3.b[k];
        }
    }
    if constexpr (KICK) {
        const float sums[7] = {st0, st1, st2, st3, st4, st5, st6};
        publish_loss_sums_kick(misc, wave, lane, sums);
    } else {
        publish_loss_sums(misc, wave, lane, st0, st1, st2, st3);
    }
    __syncthreads();
    float *slab = slabs + (long long)blockIdx.x * (KICK ? slab_stride_kick(F.total) : slab_stride(F.total));
    if (wave < 2) {
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            L1.w[k] += xch[(k)*64 + lane];
            L2.w[k] += xch[(16 + k) * 64 + lane];
            L3.w[k] += xch[(32 + k) * 64 + lane];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            L1.b[k] += xch[(48 + k) * 64 + lane];
            L2.b[k] += xch[(52 + k) * 64 + lane];
            L3.b[k] += xch[(56 + k) * 64 + lane];
        }
        if (!critic) {
            store_layer(slab, L1, lane, F.pi_w1, F.pi_b1, kH, D, D);
            store_layer(slab, L2, lane, F.pi_w2, F.pi_b2, kH, kH, kH);
            store_layer(slab, L3, lane, F.act_w, F.act_b, A, kH, kH);
        } else {
            store_layer(slab, L1, lane, F.vf_w1, F.vf_b1, kH, D, D);
            store_layer(slab, L2, lane, F.vf_w2, F.vf_b2, kH, kH, kH);
            store_layer(slab, L3, lane, F.val_w, F.val_b, 1, kH, kH);
        }
    }
    if (tid == 0) {
        if constexpr (KICK)
            store_slab_stats_kick(slab + F.total, misc);
        else
            store_slab_stats(slab + F.total, misc);
    }
