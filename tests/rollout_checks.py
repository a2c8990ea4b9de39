"""Shared by the GPU tests of the plain-shape rollout kernels (tests/test_gpu_demo_rollout.py, test_gpu_labelled_rollout.py,
test_gpu_modular_rollout.py, test_gpu_modular_labelled.py, test_gpu_preview_rollout.py, test_gpu_model_rollout.py; not a
test module): guard-byte buffers, the comparison on bits, the overflow config, the host's who-steps rule.  What is particular
to one kernel - its `sizes`, `_raw_call`, `_check_call`, `hand_collect`, `_compare_*` - stays in that kernel's file."""
import ctypes as C

import numpy as np

# a container overflows inside a three-step episode at this capacity (config.yml: 700)
OVERFLOW_OVERRIDES = {"pressing_station": {"container_capacity": 30}}


def lib():
    import marl_sortingenv_amd as M

    return M.load_library()


def cus():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


def overflow_config(noise):
    """config.yml with OVERFLOW_OVERRIDES and the sorting noise a test runs at written into it."""
    from tests import replay

    return replay.sorting_config(dict(config_overrides=OVERFLOW_OVERRIDES)).with_overrides({"sorting_station": {"noise": noise}})


def guarded(sizes):
    """Every output of `sizes` {name: bytes}, in its order, inside one byte tensor, each at a multiple of 16 with 64 guard
    bytes (0xA5) before and after it -> (raw, {name: (offset, bytes)})."""
    import torch

    at, off = {}, 64
    for name, size in sizes.items():
        at[name] = (off, size)
        off += (size + 15) // 16 * 16 + 64
    return torch.full((off,), 0xA5, dtype=torch.uint8, device="cuda:0"), at


def inside(raw, at, rows=None):
    """bool[raw.numel()]: the bytes of `guarded`'s outputs, or of each one's first rows(name, bytes) bytes."""
    import torch

    mask = torch.zeros(raw.numel(), dtype=torch.bool, device=raw.device)
    for name, (off, size) in at.items():
        mask[off:off + (size if rows is None else rows(name, size))] = True
    return mask


def bits_equal(tag, got, exp, keys, K=None):
    """got[key] and exp[key] (their first K rows where they have rows) have one shape, one dtype and the same bits."""
    import torch

    for key in keys:
        x, y = got[key], exp[key]
        if K is not None and x.dim() > 1:
            x, y = x[:K], y[:K]
        assert x.shape == y.shape and x.dtype == y.dtype, (tag, key)
        if x.dtype == torch.float32:
            x, y = x.view(torch.int32), y.view(torch.int32)
        if not torch.equal(x, y):
            bad = torch.nonzero((x != y).reshape(-1))
            raise AssertionError(f"{tag}: {key} differs at {bad.shape[0]} elements, first flat index {int(bad[0])}")


def who_host(env, mix_seed, t, threshold):
    """mse_demo_who_steps_host for the env's rows (num_envs of them from index_offset) at step t -> u8[num_envs]"""
    out = np.zeros(env.num_envs, dtype=np.uint8)
    assert env.L.mse_demo_who_steps_host(env.num_envs, env.index_offset, mix_seed, t, threshold, C.c_void_p(out.ctypes.data)) == 0
    return out
