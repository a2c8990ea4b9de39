"""CPU: the host twin of the device repack (mse_policy_pack_host: csrc/mse_policy_pack.h, the arithmetic k_policy_pack
runs too) against tests/policy_pack_reference.py, bit for bit, and the argument checks of every entry point that came
with it.  No device is touched."""
import ctypes as C

import numpy as np
import pytest

import marl_sortingenv_amd as M
from tests import policy_pack_reference as R
from marl_sortingenv_amd._lib import EXPORTS, MsePpoParams

INVALID, UNSUPPORTED = -1, -2
NEW = ("mse_policy_set_weights_device", "mse_policy_sync", "mse_policy_image_floats", "mse_policy_pack_host",
       "mse_policy_read_image", "mse_policy_get_weights", "mse_ppo_loss_grad_gated", "mse_ppo_adam_step_gated")


def _p(a):
    return C.c_void_p(a.ctypes.data)


def host_image(L, flat, D, A):
    img = np.full(int(L.mse_policy_image_floats()), np.nan, dtype=np.float32)
    ok = C.c_int32(-1)
    assert L.mse_policy_pack_host(D, A, _p(flat), _p(img), C.byref(ok)) == 0, L.mse_last_error()
    return img, bool(ok.value)


def test_layout_constants():
    L = M.load_library()
    assert L.mse_policy_image_floats() == R.IMAGE_FLOATS == 196 + 2 * 5120
    for D, A in R.SHAPES:
        assert L.mse_policy_num_weights(D, A) == R.num_weights(D, A)


@pytest.mark.parametrize("D,A", R.SHAPES)
def test_pack_host_equals_the_reference(D, A):
    L = M.load_library()
    for name, (flat, expect_ok) in R.weight_sets(D, A).items():
        want, want_ok = R.pack(flat, D, A)
        got, got_ok = host_image(L, flat, D, A)
        assert want_ok == expect_ok and got_ok == expect_ok, name
        cells = R.compared_cells(expect_ok)
        bad = np.flatnonzero(got.view(np.uint32)[cells] != want.view(np.uint32)[cells])
        assert bad.size == 0, (name, bad[:8], got[bad[:8]], want[bad[:8]])


def test_the_weight_sets_reach_their_edges():
    """what the sets are there for, shown on the reference's own image (29 -> 22)"""
    D, A = 29, 22
    img, ok = R.pack(R.weight_sets(D, A)["tiny"][0], D, A)
    assert ok
    halves = img[R.OFF_W16:].view(np.uint16)
    hi, lo = halves[:R.OPERAND_CELLS], halves[R.OPERAND_CELLS:]
    operands = img[R.OFF_W:R.OFF_W16]
    assert np.any(operands.view(np.uint32) == 0x80000000) and np.any(hi == 0x8000)  # -0 survives the fold and the split
    subnormal = lambda h: ((h & 0x7C00) == 0) & ((h & 0x3FF) != 0)
    assert np.count_nonzero(subnormal(hi)) > 50 and np.count_nonzero(subnormal(lo)) > 500
    below, _ = R.pack(R.weight_sets(D, A)["below"][0], D, A)
    assert np.max(np.abs(below[R.OFF_W:R.OFF_W16])) == np.nextafter(np.float32(65504.0), np.float32(0.0))
    above, ok = R.pack(R.weight_sets(D, A)["above"][0], D, A)
    assert not ok and np.max(np.abs(above[R.OFF_W:R.OFF_W16])) == np.float32(65504.0)


@pytest.mark.parametrize("D,A", [(13, 2), (29, 22), (1, 1)])
def test_padding_cells_are_zero(D, A):
    L = M.load_library()
    flat = R.sb3_scale(D, A, 7)
    flat[flat == 0] = 0.5  # no weight is zero: a zero cell is a padding cell
    img, ok = host_image(L, flat, D, A)
    assert ok
    halves = img[R.OFF_W16:].view(np.uint16)
    for Lr in range(5):
        for s in range(16):
            for lane in range(64):
                k, o = R.operand_input(Lr, s, lane >> 5), lane & 31
                padding = (Lr in (0, 3) and k >= D) or (Lr == 2 and o >= A)
                cells = (img[R.f32_cell(Lr, s, lane)], halves[R.f16_cell(Lr, s, lane)], halves[R.OPERAND_CELLS + R.f16_cell(Lr, s, lane)])
                assert (cells[0] == 0 and cells[1] == 0 and cells[2] == 0) == padding, (Lr, s, lane, cells)
    for h in range(2):
        for r in range(16):
            assert (img[R.OFF_B + (2 * 2 + h) * 16 + r] == 0) == (R.row_of(r, h) >= A)
    assert np.all(img[R.OFF_BV + 1:R.OFF_W].view(np.uint32) == 0)


def test_new_entry_points_check_their_arguments_without_a_device():
    L = M.load_library()
    for name in NEW:
        assert hasattr(L, name) and name in EXPORTS
    one = C.c_void_p(16)  # a non-null pointer that is never followed: every call below fails its argument checks
    flat = R.sb3_scale(13, 2, 0)
    img = np.zeros(R.IMAGE_FLOATS, np.float32)
    ok = C.c_int32(0)
    assert L.mse_policy_pack_host(13, 2, None, _p(img), C.byref(ok)) == INVALID
    assert b"mse_policy_pack_host" in L.mse_last_error()
    assert L.mse_policy_pack_host(13, 2, _p(flat), None, C.byref(ok)) == INVALID
    assert L.mse_policy_pack_host(13, 2, _p(flat), _p(img), None) == INVALID
    for D, A in ((0, 2), (33, 2), (13, 0), (13, 33)):
        assert L.mse_policy_pack_host(D, A, _p(flat), _p(img), C.byref(ok)) == UNSUPPORTED
    assert L.mse_policy_set_weights_device(None, one, None) == INVALID
    assert L.mse_policy_set_weights_device(one, None, None) == INVALID
    assert L.mse_policy_sync(None) == INVALID and b"mse_policy_sync" in L.mse_last_error()
    assert L.mse_policy_read_image(None, _p(img)) == INVALID and L.mse_policy_read_image(one, None) == INVALID
    assert L.mse_policy_get_weights(None, _p(flat)) == INVALID and L.mse_policy_get_weights(one, None) == INVALID
    p = MsePpoParams(C.sizeof(MsePpoParams), 0.2, 0.0, 0.5, 1)
    good = [29, 22, one, 64, None, 64, one, None, one, one, one, one, C.byref(p), one, one, one, None, 0.02, one]

    def call(**change):
        a = list(good)
        for k, v in change.items():
            a[int(k[1:])] = v
        return L.mse_ppo_loss_grad_gated(*a)

    assert call(a18=None) == INVALID and b"mse_ppo_loss_grad_gated" in L.mse_last_error() and b"control" in L.mse_last_error()
    assert call(a17=float("nan")) == INVALID
    assert call(a2=None) == INVALID and b"mse_ppo_loss_grad_gated" in L.mse_last_error()
    assert call(a0=0) == INVALID and call(a1=33) == INVALID and call(a5=65) == INVALID
    assert call(a13=None) == INVALID and call(a14=None) == INVALID and call(a15=None) == INVALID
    assert call(a15=C.c_void_p(24)) == -6  # MSE_ERR_ALIGNMENT
    adam = [10, one, one, one, one, 1, 3e-4, 0.9, 0.999, 1e-5, 0.5, None, None]
    assert L.mse_ppo_adam_step_gated(*adam, None) == INVALID and b"mse_ppo_adam_step_gated" in L.mse_last_error()
    assert L.mse_ppo_adam_step_gated(*([0] + adam[1:]), one) == INVALID
    assert L.mse_ppo_adam_step_gated(*(adam[:1] + [None] + adam[2:]), one) == INVALID
    assert L.mse_ppo_adam_step_gated(*(adam[:5] + [0] + adam[6:]), one) == INVALID


def test_python_surface():
    import inspect

    assert hasattr(M.MlpPolicy, "load_weights_device") and hasattr(M.MlpPolicy, "sync")
    sig = inspect.signature(M.PPOLearner.__init__).parameters
    assert sig["weight_sync"].default == "host" and sig["target_kl"].default is None
