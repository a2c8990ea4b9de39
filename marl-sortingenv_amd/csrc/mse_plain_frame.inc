// mse_plain_frame.inc -- the frame of "k_rollout_policy's plain shape" (mse_lib.hip): one wave owns 32 TILES envs for the whole
// launch, weight image(s) and tables in LDS ([weights][tables][per wave: row tile | bale ledger]), the env state in registers.
// Its five bodies - mse_rollout_policy_body.inc, k_rollout_model, mse_rollout_modular_body.inc, k_rollout_demo,
// k_rollout_policy_preview - include it four times each, MSE_PLAIN_FRAME_PART defined just before.  Before part 1 a body has
// declared, as constants and aliases only, `using L = PolLayout<...>`, `ENVS = L::ENVS` and `kWeightBytes` = L::weight_bytes x
// its weight images (0, 1 or 2); P, planes, table_image, TILES, NOISE are the kernel's.  Each part declares what its lines show.
// Text, and no statement here or between the parts may change place: why, and the three ordering rules, in DESIGN.md section 4.
#if MSE_PLAIN_FRAME_PART == 1 // carve: pointers into LDS, the wave's rows, this lane's env `i`; no memory access
    uint8_t *lds = reinterpret_cast<uint8_t *>(mse_dyn_lds);
    float *lw = reinterpret_cast<float *>(lds);
    uint32_t *ltab = reinterpret_cast<uint32_t *>(lds + kWeightBytes);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, n_waves = blockDim.x >> 6;
    const int table_bytes = P.table_words * 4;
    uint8_t *lwave = lds + kWeightBytes + table_bytes + wave * L::wave_bytes;
    uint4 *lbale = reinterpret_cast<uint4 *>(lwave + L::tile_bytes);
    const long long wave_row0 = ((long long)blockIdx.x * n_waves + wave) * ENVS;
    long long rem = P.n - wave_row0;
    const int n_valid = rem >= ENVS ? ENVS : (rem > 0 ? (int)rem : 0);
    const bool wave_active = n_valid > 0;
    // Every lane of an active wave steps an env, so that the step loop has no per-lane "is there an env here" region
    // (the compiler kept two copies of the env's ~90 registers around one and moved them back and forth every step):
    // TILES = 1: lanes 32-63 mirror lanes 0-31; lanes past the batch's end mirror its last env.  Mirrors compute what
    // their original computes and store nothing.
    const int src_lane = TILES == 1 ? (lane & 31) : lane;
    const bool live = wave_active && lane < ENVS && wave_row0 + lane < P.n;
    const long long i = wave_active ? (wave_row0 + src_lane < P.n ? wave_row0 + src_lane : P.n - 1) : 0;
#elif MSE_PLAIN_FRAME_PART == 2 // load: the tables to LDS, the wave's bale ledger (`bales`), the env `e`
    for (int w = tid; w < P.table_words / 4; w += blockDim.x)
        reinterpret_cast<uint4 *>(ltab)[w] = reinterpret_cast<const uint4 *>(table_image)[w];
    const BaleRef bales{lbale + src_lane, ENVS};
    if (P.track_bales && wave_active) {
#pragma unroll
        for (int m = 0; m < 5; ++m) lbale[m * ENVS + src_lane] = planes[(long long)(PL_BALE0 + m) * P.n_pad + i];
    }
    Env e;
    load_env<L::kind, NOISE>(e, planes, P, i);
#elif MSE_PLAIN_FRAME_PART == 3 // ready: the workgroup's barrier, waves without an env leave; `tb`
    __syncthreads();
    if (!wave_active) return;
    __builtin_amdgcn_s_waitcnt(0x0F70); // vmcnt(0): nothing but stores inside the step loop
    const Tables tb = tables_at(ltab, P);
#elif MSE_PLAIN_FRAME_PART == 4 // close: the bale ledger back to its planes
    if (P.track_bales && live) {
#pragma unroll
        for (int m = 0; m < 5; ++m) planes[(long long)(PL_BALE0 + m) * P.n_pad + i] = lbale[m * ENVS + lane];
    }
#else
#error "define MSE_PLAIN_FRAME_PART to 1, 2, 3 or 4 just before including mse_plain_frame.inc"
#endif
#undef MSE_PLAIN_FRAME_PART
