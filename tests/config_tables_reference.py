"""numpy / Python restatement of csrc/mse_tables.h: mse_config -> every Params field compile_config sets and the whole
table image, section by section, each with the reference's own expression (env_super.py / utils/input_generator.py, as
cited in the header): np.float32 casts and clips, numpy's round against Python's round for the two purity-difference
cases, np.longdouble for the tanh argument, Python integers mod 2^128 for the LCG maps.  Used by
tests/test_config_tables_cpu.py; nothing here calls the library.

Params::sr_exact_max is left out: it needs an fma, and the test checks it by property instead."""
import math

import numpy as np

OK, INVALID_ARGUMENT, UNSUPPORTED = 0, -1, -2
K_BLOCK, PAT_STRIDE, JUMP_BITS, BACK_STEPS = 256, 12, 24, 33
MASK128 = (1 << 128) - 1
PCG_MULT = 0x2360ED051FC65DA44385DF649FCCF645  # numpy's pcg64.h: PCG_DEFAULT_MULTIPLIER_HIGH / _LOW

MSG_KIND = "env_kind must be 1 (sort), 2 (press) or 3 (mono)"
MSG_MAX_STEPS = "max_steps must be in [1, 65535]"
MSG_BATCH = "input_batch_size must be in [1, 255]"
MSG_PRESS = "press_times must be in [1, 255]"
MSG_SIZES = "bale_standard_size / container_capacity / stage_capacity must be positive"
MSG_NOISE = "noise must be >= 0"
MSG_PATTERNS = "the two seasonal patterns must give distinct, non-empty material counts"
MSG_THRESHOLDS = "quality thresholds must lie in [0, 1]"
MSG_IMAGE = "container_capacity / bale_standard_size too large for the LDS-resident tables (64 KiB)"


def config_in_range(c):
    """(status, message) of the range checks, in the library's order"""
    if not 1 <= c.env_kind <= 3:
        return INVALID_ARGUMENT, MSG_KIND
    if not 1 <= c.max_steps <= 65535:
        return UNSUPPORTED, MSG_MAX_STEPS
    if not 1 <= c.input_batch_size <= 255:
        return UNSUPPORTED, MSG_BATCH
    if not (1 <= c.press_time[0] <= 255 and 1 <= c.press_time[1] <= 255):
        return UNSUPPORTED, MSG_PRESS
    if c.bale_standard_size < 1 or c.container_capacity < 1 or c.stage_capacity < 1:
        return UNSUPPORTED, MSG_SIZES
    if not c.noise >= 0.0:
        return UNSUPPORTED, MSG_NOISE
    return OK, None


# ---- bits ---------------------------------------------------------------------------------------------------------------
def f32_words(values):
    return [int(w) for w in np.asarray(values, dtype=np.float32).reshape(-1).view(np.uint32)]


def f64_words(values):
    return [int(w) for w in np.asarray(values, dtype=np.float64).reshape(-1).view(np.uint32)]  # little endian: low word first


def u64_words(v):
    return [v & 0xFFFFFFFF, (v >> 32) & 0xFFFFFFFF]


def f32_clip(v, lo, hi):
    """np.array([...], dtype=np.float32) then np.clip(obs, lo, hi) of get_sort_obs / get_press_obs"""
    return np.clip(np.float32(v), np.float32(lo), np.float32(hi))


# ---- the LCG as Python integers ----------------------------------------------------------------------------------------
def lcg_forward(n):
    """(a, g) of n >= 0 steps s' = M s + inc: a = M^n, g = (M^n - 1) / (M - 1).  M - 1 = 4 x odd, so the quotient is
    taken mod 2^130 and the odd part inverted mod 2^128."""
    assert (PCG_MULT - 1) % 4 == 0 and ((PCG_MULT - 1) // 4) % 2 == 1
    a = pow(PCG_MULT, n, 1 << 128)
    g = ((pow(PCG_MULT, n, 1 << 130) - 1) // 4) * pow((PCG_MULT - 1) // 4, -1, 1 << 128) & MASK128
    return a, g


def lcg_backward(d):
    """the inverse of d steps: s = a^-1 (s' - g inc)"""
    a, g = lcg_forward(d)
    inv = pow(a, -1, 1 << 128)
    return inv, (-inv * g) & MASK128


def lcg_apply(f, s, inc):
    return (f[0] * s + f[1] * inc) & MASK128


def map_words(f):
    return u64_words(f[0] & (2**64 - 1)) + u64_words(f[0] >> 64) + u64_words(f[1] & (2**64 - 1)) + u64_words(f[1] >> 64)


# ---- the config compiler ----------------------------------------------------------------------------------------------
def max_draws_per_step(baseline, boost, noise, counts, kind):
    """mse_plan.h: the mis-sorted units of a step at the lowest accuracy the noise allows, over patterns and modes"""
    worst = 0
    for k in (1, 2):
        for mode in range(3 if kind == 2 else 2):
            s = 0
            for m in range(4):
                boosted = (mode == 0 and m in (0, 2)) or (mode == 1 and m in (1, 3))
                acc = min(1.0, max(0.0, baseline[m] + (boost if boosted else 0.0) - noise))
                s += counts[k][m] - int(np.rint(counts[k][m] * acc))
            worst = max(worst, s)
    return worst


def compile_config(c, n_envs, index_offset):
    """-> (status, message, params dict, image word list, literal, noise_on); the last four are None on a refusal"""
    cap, S, batch, stage = c.container_capacity, c.bale_standard_size, c.input_batch_size, c.stage_capacity
    baseline = [c.baseline_accuracy[m] for m in range(4)]
    thr = [c.quality_threshold[m] for m in range(4)]
    thr_r2 = [c.quality_threshold_r2[m] for m in range(4)]
    refusal = lambda msg: (UNSUPPORTED, msg, None, None, None, None)

    P = dict(n=n_envs, n_pad=(n_envs + K_BLOCK - 1) // K_BLOCK * K_BLOCK, index_offset=index_offset,
             env_kind=c.env_kind, max_steps=c.max_steps, auto_reset=int(c.auto_reset != 0),
             track_bales=int(c.track_bales != 0), balesize=S, capacity=cap, stage_capacity=stage, batch=batch,
             press_time=[c.press_time[0], c.press_time[1]], press_time0=c.press_time[0], press_time1=c.press_time[1],
             inv_balesize=np.float32(1.0) / np.float32(S), max_state_reward=c.max_state_reward)
    # env_super.py:664-666: the stored bale quality int(q * 100) of q = k / 100
    qi_down = [0, 0, 0, 0]
    for q in range(101):
        if int((q / 100.0) * 100.0) != q:
            assert int((q / 100.0) * 100.0) == q - 1
            qi_down[q >> 5] |= 1 << (q & 31)
    P["qi_down"] = qi_down
    P["rem_thr_units"] = math.floor(S * c.bale_remainder_threshold)
    P["sr_den"] = float(5 * cap)
    P["sr_inv"] = 1.0 / P["sr_den"]

    # utils/input_generator.py:46-55: int(np.floor(ratio * batchsize)) per material; key 0 = the empty stage after reset
    counts = [[0, 0, 0, 0]] + [[int(np.floor(c.pattern_ratio[k][m] * batch)) for m in range(4)] for k in range(2)]
    P["pat_word"] = [sum(cnt[m] << (8 * m) for m in range(4)) & 0xFFFFFFFF for cnt in counts]
    P["pat_word1"], P["pat_word2"] = P["pat_word"][1], P["pat_word"][2]
    P["gen_rem"] = [0] + [batch - sum(cnt) for cnt in counts[1:]]
    P["gen_mode"] = int(any(r != 0 for r in P["gen_rem"]))
    P["occ_nonempty"] = f32_words(f32_clip(round(batch / 100, 2), -1, 1))[0]  # env_super.py:456, :318-325
    pat = []
    for word, cnt in zip(P["pat_word"], counts):
        total = sum(cnt)
        prop = [x / total if total > 0 else 0 for x in cnt]                      # env_super.py:199-210
        mode = 0 if prop[0] + prop[2] > prop[1] + prop[3] else 1                 # env_super.py:479-482
        pat += [word, f32_words(f32_clip(round(total / 100, 2), -1, 1))[0], mode, 0]
        pat += f32_words([f32_clip(x, -1, 1) for x in prop])
        pat += f32_words([f32_clip(x / stage, 0, 1) for x in cnt])               # env_super.py:351, :358-359
    if not P["gen_mode"] and (P["pat_word"][1] == P["pat_word"][2] or 0 in P["pat_word"][1:]):
        return refusal(MSG_PATTERNS)

    # env_super.py:1020-1027: the levels whose fill_ratio is above 0.95 / 0.90 start one past the threshold
    P["sev_negative"], P["mild_negative"] = int(c.overflow_penalty_severe < 0), int(c.overflow_penalty_mild < 0)
    P["thr_sev"] = min(L for L in range(cap + 1) if L / cap > 0.95) - 1
    P["thr_mild"] = min(L for L in range(cap + 1) if L / cap > 0.90) - 1
    P["k_thr"] = [int(np.rint(t * 100.0)) for t in thr_r2]
    if any(not 0 <= k <= 100 for k in P["k_thr"]):
        return refusal(MSG_THRESHOLDS)
    # env_super.py:499-509 without the noise: mode 0 boosts A and C, mode 1 B and D, any other mode nothing
    acc_rows = []
    for boosted in ((0, 2), (1, 3), ()):
        acc = list(baseline)
        for m in boosted:
            acc[m] += c.boost
        acc_rows.append(np.clip(np.array(acc) + 0.0, 0, 1))
    P["acc_floor"] = [float(min(np.clip(baseline[m] - c.noise, 0, 1), np.clip(baseline[m] + c.boost - c.noise, 0, 1)))
                      for m in range(4)]

    img = []
    P["off_lvl"] = len(img)
    img += f32_words([f32_clip(L / cap, 0, 1) for L in range(cap + 1)])          # env_super.py:339-344, :358-359
    P["off_pdiff"] = len(img)
    for m in range(4):
        # env_super.py:212-227 with :784-789: a filled container's purity is a rounded np.float64 quotient and the
        # difference is rounded by numpy; an empty container's is round(threshold, 2) of a Python float and the
        # difference is rounded by Python
        diffs = [round(np.float64(k / 100.0) - thr[m], 2) for k in range(101)] + [round(thr_r2[m] - thr[m], 2)]
        assert all(type(d) is np.float64 for d in diffs[:101]) and type(diffs[101]) is float
        img += f32_words([f32_clip(d, -1, 1) for d in diffs])
    for i in range(2):                                                           # env_super.py:354-359
        P["off_timer%d" % i] = len(img)
        img += f32_words([f32_clip(t / c.press_time[i], 0, 1) for t in range(c.press_time[i] + 1)])
    img += [0] * (len(img) % 2)
    P["off_tanh"] = len(img)
    ld = np.longdouble
    for s in range(401):                                                         # env_super.py:963-1003 by purity sum
        total = ld(s) / ld(100) - ld(4) * ld(c.purity_threshold_theta)
        state_based = float((total / ld(4)) * ld(2))
        img += f64_words(math.tanh(state_based / c.tanh_temperature))
    P["off_eff"] = len(img)
    img += f64_words([(1.0 - 4.0 * (d / S)) * c.bale_efficiency_factor for d in range(S // 2 + 1)])  # env_super.py:1058-1062
    P["off_acc"] = len(img)
    img += f64_words(np.concatenate(acc_rows))
    P["off_bonus"] = len(img)
    img += f64_words(np.array([0.0, 1 / 3, 2 / 3, 1.0]) - c.bale_efficiency_factor)                   # env_super.py:1065-1069
    img += [0] * (-len(img) % 4)
    P["off_pat"] = len(img)
    assert len(pat) == 3 * PAT_STRIDE
    img += pat
    P["off_ptime"] = len(img)
    img += [c.press_time[0], c.press_time[1]] + qi_down
    P["off_cst"] = len(img)
    img += f64_words([c.overflow_penalty_catastrophic, c.overflow_penalty_severe, c.overflow_penalty_mild,
                      c.max_state_reward, c.overflow_termination_penalty, c.bale_remainder_threshold, c.boost, c.noise]
                     + baseline)
    img += [0] * (-len(img) % 4)
    P["off_jump"] = len(img)
    for j in range(JUMP_BITS):
        img += map_words(lcg_forward(1 << j))
    P["off_back"] = len(img)
    for d in range(BACK_STEPS):
        img += map_words(lcg_backward(d))
    P["off_gprop"] = P["off_gfrac"] = 0
    if P["gen_mode"]:
        P["off_gprop"] = len(img)
        img += f32_words([f32_clip(k / batch, -1, 1) for k in range(256)])
        P["off_gfrac"] = len(img)
        img += f32_words([f32_clip(k / stage, 0, 1) for k in range(256)])
    img += [0] * (-len(img) % 4)
    P["table_words"] = len(img)
    if len(img) > 16384:
        return refusal(MSG_IMAGE)

    P["ring_worst"] = max_draws_per_step(baseline, c.boost, c.noise, counts, c.env_kind)
    fwd = lcg_forward(P["ring_worst"])
    P["ring_fwd"] = [fwd[0] & (2**64 - 1), fwd[0] >> 64, fwd[1] & (2**64 - 1), fwd[1] >> 64]
    literal = c.literal_choice != 0 or batch > 127
    return OK, None, P, img, literal, c.noise != 0.0
