// mse_ppo_matrix_body.inc -- the statements of k_ppo_grad_matrix's body (mse_ppo_matrix.hip), included once per __global__
// entry of the kernel: k_ppo_grad_matrix (KICK = false) and k_ppo_grad_matrix_kick (KICK = true).  Text and not a function for
// the reason mse_ppo_grad_body.inc gives.  The including function provides the template parameters DP, AP, VCLIP, the
// constants BC and KICK, the kernel's arguments and `K` (KickArgs; never read with KICK = false).  Likewise
// k_ppo_grad_matrix_shard (SHARD = true) with `S` (ShardArgs; never read with SHARD = false), as in mse_ppo_grad_body.inc.
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
    float *misc = strips + 4 * kStripFloats; // kMiscFloats (KICK: kKickMiscFloats)
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
    if constexpr (SHARD)
        publish_shard_mean_std(G, S, misc, wave, lane);
    else
        publish_adv_mean_std(G, rows, adv, adv_partial, misc, wave, lane);
    __syncthreads();
    const bool normalize = G.n_adv_partial > 0;
    const float mean = misc[0], std = misc[1];
    const float inv_b_all = 1.0f / (float)(SHARD ? S.global_batch : G.batch); // SHARD: G.batch is the local row bound
    const bool critic = (wave & 1) != 0;
    float *strip = strips + wave * kStripFloats;
    LayerGrad L1, L2, L3; // first, second hidden layer, head
#pragma unroll
    for (int r = 0; r < 16; ++r) L1.w[r] = L2.w[r] = L3.w[r] = 0.0f;
    L1.b = L2.b = L3.b = 0.0f;
    float st0 = 0.0f, st1 = 0.0f, st2 = 0.0f, st3 = 0.0f;
    [[maybe_unused]] float st4 = 0.0f, st5 = 0.0f, st6 = 0.0f; // KICK only
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
            if constexpr (KICK) {
                const int action = clamped_action(actions[row], A);
                const float a_raw = adv[row];
                const float a_used = normalize ? normalized_advantage(a_raw, mean, std) : a_raw;
                const PolicyBcTerms kt =
                    policy_bc_head_terms<AP>(dl, A, legal, action, K.expert_actions[row], old_logp[row], a_used, G.P, K.bc_coef, inv_b);
                if (valid) {
                    st0 += kt.surrogate;
                    st1 += kt.entropy;
                    st2 += kt.kl;
                    st3 += kt.clipped;
                    st4 += kt.ce;
                    st5 += kt.hit;
                    st6 += kt.unusable;
                }
            } else if constexpr (BC) {
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
    if constexpr (KICK) {
        st4 = wave_sum(st4);
        st5 = wave_sum(st5);
        st6 = wave_sum(st6);
    }
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
    if (tid == 0) {
        if constexpr (KICK)
            store_slab_stats_kick(slab + F.total, misc);
        else
            store_slab_stats(slab + F.total, misc);
    }
