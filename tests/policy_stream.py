"""Host restatement of the on-device policy stream (csrc/mse_policy_stream.h), vectorised in NumPy, and of the
masked-uniform random policy that draws from it (policy_action in csrc/mse_lib.hip).

One 32-bit word per (policy seed, global env index, step counter t): key = mse_policy_key(seed, index),
word = mse_policy_word(key, t).  All arithmetic is on uint32 / uint64 arrays, so a whole batch of envs is one call."""
from __future__ import annotations

import numpy as np

_M32 = np.uint64(0xFFFFFFFF)


def _u32(x):
    return np.asarray(x, dtype=np.uint64) & _M32


def fmix32(h):
    """murmur3's 32-bit finaliser on a uint32 / uint64 array (values < 2**32) -> uint64 array of 32-bit values."""
    h = _u32(h)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & _M32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & _M32
    h ^= h >> np.uint64(16)
    return h


def policy_key(seed: int, env_index) -> np.ndarray:
    """mse_policy_key(seed, env_index): seed a Python int in [0, 2**64), env_index an int array (global indices)."""
    seed = int(seed) % 2**64
    s = int(fmix32(np.uint64(seed & 0xFFFFFFFF) ^ fmix32(((seed >> 32) + 0x9E3779B9) & 0xFFFFFFFF)))
    g = np.asarray(env_index, dtype=np.uint64)
    gw = (_u32(g) * np.uint64(0x9E3779B1) + (g >> np.uint64(32)) * np.uint64(0xC2B2AE3D)) & _M32
    return fmix32((np.uint64(s) + gw) & _M32)


def policy_word(key, t: int) -> np.ndarray:
    """mse_policy_word(key, t) for a key array and one step counter t."""
    t = int(t) % 2**64
    c = ((t & 0xFFFFFFFF) * 0x85EBCA77 + (t >> 32) * 0x27D4EB2F) & 0xFFFFFFFF
    return fmix32(np.uint64(c) ^ _u32(key))


def word(seed: int, env_index, t: int) -> np.ndarray:
    return policy_word(policy_key(seed, env_index), t)


def masked_uniform(words, mask, use_action_masking: bool = True) -> np.ndarray:
    """The random policy's action: the k-th valid action of mask [N, A] with k = (w * count) >> 32, or
    (w * A) >> 32 over the whole action space without masking -> int32 [N]."""
    mask = np.asarray(mask).astype(bool)
    n, A = mask.shape
    w = _u32(words)
    if not use_action_masking:
        return ((w * np.uint64(A)) >> np.uint64(32)).astype(np.int32)
    cnt = mask.sum(axis=1).astype(np.uint64)
    k = ((w * cnt) >> np.uint64(32)).astype(np.int64)
    # position of the (k+1)-th set bit: the first column whose running count exceeds k
    run = np.cumsum(mask, axis=1)
    return np.argmax(run > k[:, None], axis=1).astype(np.int32)


def uniform24(words) -> np.ndarray:
    """The policy network's categorical draw u = (w >> 8) * 2**-24 in [0, 1), as float64."""
    return (_u32(words) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
