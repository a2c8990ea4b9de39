// mse_params.h -- what the host and the kernels both read: the kernel-argument block `Params` and the shape of the
// lookup-table image.  No HIP here: mse_tables.h (compile_config) fills both on the host, mse_device.h reads them on
// the device, and tests/test_config_tables_cpu.py compiles the host side with the host compiler.
#pragma once

#include <stdint.h>

namespace mse {

constexpr int kBlock = 256;             // threads per workgroup = 4 wavefronts of 64

constexpr int kPdiffStride = 102; // purity hundredths 0..100, [101] = empty container
// per-stage-id record in the LDS table image (12 words, 16-byte aligned):
//   [0] packed counts  [1] belt_occupancy f32  [2] sorting_rules() mode  [3] pad
//   [4..7] belt proportions f32   [8..11] sorting[m]/stage_capacity f32
constexpr int kPatStride = 12;

// fp64 constants kept in the LDS table image (Tables::cst)
enum Cst : int { CST_PEN_CAT = 0, CST_PEN_SEV, CST_PEN_MILD, CST_MAX_STATE, CST_OVERFLOW_PEN, CST_REM_THR, CST_BOOST,
                 CST_NOISE, CST_BASE_ACC0, CST_BASE_ACC1, CST_BASE_ACC2, CST_BASE_ACC3, CST_COUNT };

constexpr int kJumpBits = 24;      // entries of the LCG jump-ahead table: 2^j steps, j = 0..23 (pcg_jump)
constexpr int kRingBackSteps = 33; // entries of the jump-back table: d = 0..32 steps (pcg_step_back)

struct Params {
    long long n;            // envs in this handle
    long long n_pad;        // plane stride (multiple of kBlock)
    long long index_offset; // global index of env 0 (sharded runs)
    int env_kind, max_steps, auto_reset, track_bales;
    int balesize, capacity, stage_capacity, batch;
    int press_time[2];
    int press_time0, press_time1; // the same as two scalars: selected per lane with v_cndmask, never indexed
    float inv_balesize;           // 1.0f / bale_standard_size (quotient estimate, fixed up exactly)
    double max_state_reward;      // used every step: stays a kernel argument (SGPR pair)
    double sr_den, sr_inv;        // 5 * capacity and its reciprocal (state_ratio)
    int sr_exact_max;             // state_ratio's reciprocal form is proven for 0 <= total_level <= this
    // stage vectors are one of three words: id 0 = empty (after reset), 1 / 2 = seasonal pattern
    uint32_t pat_word[3];   // packed u8x4 counts A..D (load/store conversion)
    uint32_t pat_word1, pat_word2; // the same as two scalars: a per-lane choice between them is two v_cndmask on
                                   // SGPRs (indexing the array per lane would be a global load)
    int thr_sev, thr_mild;  // levels above these have fill_ratio > 0.95 / > 0.90 (literal fp64 scan on the host)
    int sev_negative, mild_negative; // overflow_penalty_severe / _mild < 0 (then that bracket returns early)
    int k_thr[4];           // hundredths of python round(quality_threshold, 2): purity of an empty container
    // offsets (in 4-byte words) into the table image; see compile_config (mse_tables.h)
    int off_lvl, off_pdiff, off_timer0, off_timer1, off_tanh, off_eff, off_pat, off_acc, off_bonus, off_ptime, off_cst, off_jump, off_back, table_words;
    uint32_t qi_down[4]; // bit q set: int((q / 100.0) * 100.0) == q - 1  (press_bale's stored quality)
    int rem_thr_units;   // floor(bale_standard_size * bale_remainder_threshold)
    int ring_worst; // most sort_material draws one step can make with this config (k_rollout_ring flow control)
    // the LCG's jump FORWARD by ring_worst steps, s' = A s + G inc (A_lo, A_hi, G_lo, G_hi): the two halves of the
    // ring's priming are that far apart (k_rollout_ring); kernel arguments because the observer lanes need them
    // before the table image is in LDS
    uint64_t ring_fwd[4];
    // General generator mode (utils/input_generator.py:46-61 with a floor() remainder, e.g. input_batch_size 90): the stage
    // vectors are carried as their packed counts instead of pattern ids, the generator's private stream runs on the
    // device (remainder draws + the shuffle's draws), and only the one-lane kernels serve the handle.
    int gen_mode;
    int gen_rem[3];            // units left after the floor()s, per pattern key (index 1 | 2)
    uint32_t occ_nonempty;     // f32 bits of clip(float(round(batch / 100, 2))): occupancy of a stage that holds a batch
    int off_gprop, off_gfrac;  // tables by count: clip(float(k / batch)), clip(float(k / stage_capacity)), k = 0..255
    double acc_floor[4]; // lowest accuracy_belt[m] the config can produce: clip(baseline [+ boost] - noise).  ring_worst
                         // is derived from it, so mse_set_state counts anything below as an error (mse_error_count)
};

} // namespace mse
