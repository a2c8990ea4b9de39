"""The learner's counter-based minibatch permutation restated in numpy, from the comment above `shuffle_key` in
marl-sortingenv_amd/csrc/mse_ppo_math.h alone (it never calls the library): the independent yardstick of
tests/test_ppo_shuffle_cpu.py.  All arithmetic is uint32 and wraps."""
import numpy as np

ROUNDS = 6
GOLDEN = 0x9E3779B9
ROUND_STEP = 0x85EBCA77
M32 = 0xFFFFFFFF


def mix32(h):
    """murmur3's 32-bit finaliser on a uint32 array (or Python int)."""
    if isinstance(h, int):
        h ^= h >> 16
        h = (h * 0x85EBCA6B) & M32
        h ^= h >> 13
        h = (h * 0xC2B2AE35) & M32
        return h ^ (h >> 16)
    h = h.astype(np.uint32)
    h = h ^ (h >> np.uint32(16))
    h = h * np.uint32(0x85EBCA6B)
    h = h ^ (h >> np.uint32(13))
    h = h * np.uint32(0xC2B2AE35)
    return h ^ (h >> np.uint32(16))


def round_keys(seed: int, epoch: int):
    """The six round keys of (seed, epoch), both uint64."""
    h = GOLDEN
    for w in (seed & M32, (seed >> 32) & M32, epoch & M32, (epoch >> 32) & M32):
        h = mix32(((h ^ w) + GOLDEN) & M32)
    return [mix32(h ^ (((r + 1) * ROUND_STEP) & M32)) for r in range(ROUNDS)]


def bits_of(total: int):
    b = max(2, (total - 1).bit_length())
    lo = b // 2
    return b - lo, lo  # (bits of the high half, bits of the low half)


def _encrypt(x, keys, hi_bits, lo_bits):
    lo_mask, hi_mask = np.uint32((1 << lo_bits) - 1), np.uint32((1 << hi_bits) - 1)
    hi, lo = x >> np.uint32(lo_bits), x & lo_mask
    for r, k in enumerate(keys):
        if r % 2 == 0:
            hi = hi ^ (mix32(lo ^ np.uint32(k)) & hi_mask)
        else:
            lo = lo ^ (mix32(hi ^ np.uint32(k)) & lo_mask)
    return (hi << np.uint32(lo_bits)) | lo


def permutation(total: int, seed: int, epoch: int, first: int = 0, count=None) -> np.ndarray:
    """perm(seed, epoch, total, i) for i in [first, first + count) as int64."""
    assert 1 <= total <= 2 ** 31
    count = total - first if count is None else count
    keys = round_keys(seed, epoch)
    hi_bits, lo_bits = bits_of(total)
    with np.errstate(over="ignore"):
        x = _encrypt(np.arange(first, first + count, dtype=np.int64).astype(np.uint32), keys, hi_bits, lo_bits)
        while True:  # cycle walking: re-apply while the value lies outside [0, total)
            out = np.nonzero(x.astype(np.int64) >= total)[0]
            if out.size == 0:
                return x.astype(np.int64)
            x[out] = _encrypt(x[out], keys, hi_bits, lo_bits)
