"""numpy restatement of the top comment of csrc/mse_policy_pack.h: flat torch.nn.Linear weights -> the packed policy
image.  float64 fold with sequential sums, the operand order the accumulator registers impose, the layout offsets, and
the f16 hi / lo split on integers.  Shared by tests/test_policy_pack_cpu.py and tests/test_gpu_policy_pack.py; nothing
here calls the library."""
import numpy as np

H = 32
OFF_B, OFF_WV, OFF_BV = 0, 5 * 32, 5 * 32 + 32
OFF_W = (OFF_BV + 1 + 3) // 4 * 4
OPERAND_CELLS = 5 * 16 * 64
OFF_W16 = OFF_W + OPERAND_CELLS          # in f32 cells; the section holds 2 * OPERAND_CELLS 16-bit cells
IMAGE_FLOATS = OFF_W16 + OPERAND_CELLS
C2 = 2.0 * 1.4426950408889634            # 2 log2 e
HALF_LIMIT = np.float32(65504.0)
SHAPES = ((13, 2), (16, 11), (29, 22), (1, 1), (32, 32))


def num_weights(D, A):
    return 2 * (H * D + H + H * H + H) + A * H + A + H + 1


def split(flat, D, A):
    sizes = [H * D, H, H * H, H, A * H, A, H * D, H, H * H, H, H, 1]
    shapes = [(H, D), (H,), (H, H), (H,), (A, H), (A,), (H, D), (H,), (H, H), (H,), (H,), (1,)]
    parts = np.split(np.asarray(flat, dtype=np.float32), np.cumsum(sizes)[:-1])
    return [p.reshape(s) for p, s in zip(parts, shapes)]


def row_of(r, h):
    return (r & 3) + 8 * (r >> 2) + 4 * h


def _row_sums(w):
    """S[o] = 0.0 + w[o, 0] + w[o, 1] + ... in that order, one float64 add each (np.sum would add pairwise)."""
    s = np.zeros(w.shape[0], dtype=np.float64)
    for i in range(w.shape[1]):
        s = s + w[:, i].astype(np.float64)
    return s


def fold(flat, D, A):
    """(Wf f64[5, 32, 32], Bf f64[5, 32], wv f64[32], bv f64): step 1 of the header comment."""
    pi_w1, pi_b1, pi_w2, pi_b2, act_w, act_b, vf_w1, vf_b1, vf_w2, vf_b2, val_w, val_b = \
        [p.astype(np.float64) for p in split(flat, D, A)]
    Wf, Bf = np.zeros((5, 32, 32)), np.zeros((5, 32))
    for L, (w1, b1, w2, b2) in ((0, (pi_w1, pi_b1, pi_w2, pi_b2)), (3, (vf_w1, vf_b1, vf_w2, vf_b2))):
        Wf[L, :, :D] = C2 * w1
        Bf[L] = C2 * b1
        Wf[L + 1] = (-2.0 * C2) * w2
        Bf[L + 1] = C2 * (b2 + _row_sums(w2))
    Wf[2, :A] = -2.0 * act_w
    Bf[2, :A] = act_b + _row_sums(act_w)
    return Wf, Bf, -2.0 * val_w, val_b[0] + _row_sums(val_w[None, :])[0]


def half_rtz(v):
    """f32 array -> f16 bit patterns (u16), rounded toward zero, on the bits."""
    u = np.asarray(v, dtype=np.float32).view(np.uint32).astype(np.int64)
    sg = (u >> 16) & 0x8000
    E = (u >> 23) & 0xFF
    e = E - 127
    m = (u & 0x7FFFFF) | 0x800000
    normal = sg | ((e + 15) << 10) | ((m >> 13) & 0x3FF)
    sub = sg | (m >> np.clip(13 + (-14 - e), 0, 63))
    out = np.where(E == 0, sg, np.where(e >= -14, normal, np.where(e < -25, sg, sub)))
    return out.astype(np.uint16)


def half_value(bits):
    return np.asarray(bits, dtype=np.uint16).view(np.float16).astype(np.float64)  # every f16 is a float64


def half_rne(v):
    """to nearest: the truncated value t or the next magnitude u = t + 1, whichever is closer, ties to the even pattern"""
    v = np.asarray(v, dtype=np.float32)
    t = half_rtz(v)
    u = (t + np.uint16(1)).astype(np.uint16)
    da = np.abs(v.astype(np.float64) - half_value(t))
    db = np.abs(half_value(u) - v.astype(np.float64))
    return np.where((db < da) | ((db == da) & ((u & 1) == 0)), u, t).astype(np.uint16)


def f32_cell(L, s, lane):
    return OFF_W + ((4 * L + (s >> 2)) * 64 + lane) * 4 + (s & 3)


def f16_cell(L, s, lane):
    return ((2 * L + (s >> 3)) * 64 + lane) * 8 + (s & 7)  # hi; lo is OPERAND_CELLS further


def operand_input(L, s, hp):
    return 2 * s + hp if L in (0, 3) else row_of(s, hp)


def pack(flat, D, A):
    """-> (image f32[IMAGE_FLOATS], f16_ok).  Without f16_ok the f16 section is left zero: it is unspecified."""
    Wf, Bf, wv, bv = fold(flat, D, A)
    W32, B32 = Wf.astype(np.float32), Bf.astype(np.float32)
    img = np.zeros(IMAGE_FLOATS, dtype=np.float32)
    for L in range(5):
        for h in range(2):
            for r in range(16):
                img[OFF_B + (2 * L + h) * 16 + r] = B32[L, row_of(r, h)]
    for h in range(2):
        for r in range(16):
            img[OFF_WV + h * 16 + r] = np.float32(wv[row_of(r, h)])
    img[OFF_BV] = np.float32(bv)
    wf = np.zeros(OPERAND_CELLS, dtype=np.float32)  # in f16_cell order
    for L in range(5):
        for s in range(16):
            for lane in range(64):
                v = W32[L, lane & 31, operand_input(L, s, lane >> 5)]
                img[f32_cell(L, s, lane)] = v
                wf[f16_cell(L, s, lane)] = v
    f16_ok = bool(np.all(np.abs(wf) < HALF_LIMIT))
    if f16_ok:
        hi = half_rtz(wf)
        lo = half_rne(wf - hi.view(np.float16).astype(np.float32))  # the f32 subtraction is exact
        img[OFF_W16:].view(np.uint16)[:] = np.concatenate([hi, lo])
    return img, f16_ok


def compared_cells(f16_ok):
    """the cells of an image that are specified: all of it, or all but the f16 section"""
    return slice(0, IMAGE_FLOATS if f16_ok else OFF_W16)


# ---- weight sets ---------------------------------------------------------------------------------------------------------
def sb3_scale(D, A, seed):
    """SB3's initial magnitudes (MlpPolicy.random_init) with non-zero biases"""
    rng = np.random.default_rng(seed)
    parts = []
    for i, p in enumerate(split(np.zeros(num_weights(D, A), np.float32), D, A)):
        if p.ndim == 1 and i != 10:
            parts.append(rng.standard_normal(p.shape) * 0.1)
        else:
            gain = 0.01 if i == 4 else (1.0 if i == 10 else np.sqrt(2.0))
            parts.append(rng.standard_normal(p.shape) * gain / np.sqrt(p.shape[-1]))
    return np.concatenate([p.ravel() for p in parts]).astype(np.float32)


def tiny_and_zero(D, A, seed):
    """0, -0 and magnitudes from 1 down to 1e-9: hi parts that are f16 subnormals or vanish (below 2^-25), lo parts
    that are f16 subnormals (every folded weight below 2^-4 has one)"""
    rng = np.random.default_rng(seed)
    w = sb3_scale(D, A, seed + 1).astype(np.float64)
    w *= 10.0 ** -rng.choice([0, 3, 6, 9], size=w.size)
    kind = rng.integers(0, 8, size=w.size)
    w[kind == 0] = 0.0
    w[kind == 1] = -0.0
    return w.astype(np.float32)


def at_the_f16_limit(D, A, seed, above):
    """one action-head weight whose fold (-2 w, exact) is the f32 just below 65 504 in magnitude, or, `above`, 65 504
    itself - the first value that does not fit"""
    w = sb3_scale(D, A, seed)
    at = H * D + H + H * H + H + min(3, H - 1)  # act_w[0, 3]
    w[at] = np.float32(32752.0) if above else np.nextafter(np.float32(32752.0), np.float32(0.0))
    return w


def weight_sets(D, A):
    """name -> (flat weights, the f16_ok they must give)"""
    return {"sb3": (sb3_scale(D, A, 1), True), "tiny": (tiny_and_zero(D, A, 2), True),
            "below": (at_the_f16_limit(D, A, 3, False), True), "above": (at_the_f16_limit(D, A, 3, True), False)}
