"""CPU: the ABI of the preview rollout (include/mse.h: mse_preview_buffers, mse_rollout_policy_preview) and its shape.

  * the ctypes mirror MsePreviewBuffers has the size and the field order the header declares: a few lines of C compiled
    against include/mse.h print sizeof and every offsetof;
  * plan_policy_plain (csrc/mse_plan.h, compiled on the host) gives the entry - one network, Env_3's tiles - the plain
    policy kernel's LDS bytes, wave shape and grid at 1, 256 x CUs and 256 x CUs + 1 envs, in both precision forms;
  * the entry's launch is planned by that call (the source says so) and the constants Python restates are the header's.
"""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "marl-sortingenv_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")

FIELDS = ("observations", "action_masks", "episode_starts", "actions", "log_probs", "values", "rewards", "expert_actions",
          "stepped_actions", "expert_stepped", "last_values", "last_dones")

LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "mse.h"
int main(void)
{
    printf("sizeof %zu\n", sizeof(mse_preview_buffers));
    printf("struct_size %zu\n", offsetof(mse_preview_buffers, struct_size));
    printf("reserved0 %zu\n", offsetof(mse_preview_buffers, reserved0));
@FIELDS@
    printf("MSE_PREVIEW_DETERMINISTIC %u\n", MSE_PREVIEW_DETERMINISTIC);
    return 0;
}
""".replace("@FIELDS@", "\n".join(f'    printf("{f} %zu\\n", offsetof(mse_preview_buffers, {f}));' for f in FIELDS))

PLAN_SHIM = r"""
#include "mse_plan.h"
using namespace mse;
static void out(const PolicyPlan &p, long long *o)
{
    o[0] = p.status; o[1] = (long long)p.kernel; o[2] = (long long)p.lds_bytes; o[3] = p.tiles; o[4] = p.n_waves; o[5] = p.workgroups;
}
static PolicyLds lds_of(const unsigned long long *l) { return {l[0], l[1], l[2], l[3], {l[4], l[5]}}; }
extern "C" {
void preview(long long n, int cus, int f16, const unsigned long long *lds, long long *o)
{
    out(plan_policy_plain(n, cus, f16 != 0, 1, lds_of(lds)), o);
}
// mse_rollout_policy held to the plain kernel: rollout_pipeline = 2, no sorting policy
void plain(long long n, int cus, int f16, const unsigned long long *lds, long long *o)
{
    out(plan_rollout_policy(2, n, cus, f16 != 0, false, 0, false, false, true, lds_of(lds)), o);
}
}
"""


def _compiler(*names):
    for name in names:
        path = shutil.which(name)
        if path is not None:
            return path
    pytest.fail(f"no host compiler among {names}")


def test_ctypes_mirror_has_the_headers_layout(tmp_path):
    from marl_sortingenv_amd._lib import MSE_PREVIEW_DETERMINISTIC, PREVIEW_BUFFER_NAMES, MsePreviewBuffers

    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_C)
    subprocess.run([_compiler("gcc", "cc", "clang"), "-std=c99", "-I", INCLUDE, str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    said = {k: int(v) for k, v in (line.split() for line in lines if line)}
    assert PREVIEW_BUFFER_NAMES == FIELDS
    assert C.sizeof(MsePreviewBuffers) == said["sizeof"] == 8 + 8 * len(FIELDS)
    assert [name for name, _ in MsePreviewBuffers._fields_] == ["struct_size", "reserved0"] + list(FIELDS)
    for name, _ in MsePreviewBuffers._fields_:
        assert getattr(MsePreviewBuffers, name).offset == said[name], name
    # the header declares the members in the order the kernel's sentence names them
    order = sorted(FIELDS, key=lambda f: said[f])
    assert tuple(order) == FIELDS
    assert MSE_PREVIEW_DETERMINISTIC == said["MSE_PREVIEW_DETERMINISTIC"] == 1024


def test_preview_flag_is_no_other_flag():
    text = open(os.path.join(INCLUDE, "mse.h")).read()
    flags = {name: int(v) for name, v in re.findall(r"#define\s+(MSE_(?:STEP|ROLLOUT|MODEL|MODULAR|DEMO|PREVIEW)_[A-Z_]+)\s+(\d+)u", text)}
    assert flags["MSE_PREVIEW_DETERMINISTIC"] == 1024
    values = list(flags.values())
    assert len(set(values)) == len(values), flags


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    d = tmp_path_factory.mktemp("preview_plan")
    src, so = d / "shim.cpp", d / "shim.so"
    src.write_text(PLAN_SHIM)
    subprocess.run([_compiler("c++", "g++", "clang++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, "-I", INCLUDE,
                    str(src), "-o", str(so)], check=True)
    L = C.CDLL(str(so))
    for fn in (L.preview, L.plain):
        fn.argtypes = [C.c_longlong, C.c_int, C.c_int, C.POINTER(C.c_ulonglong), C.POINTER(C.c_longlong)]
        fn.restype = None
    return L


# PolLayout<3, TILES> (mse_lib.hip): a wave's 29-float observation tile, rounded to 16 bytes, and its 5-plane bale ledger
WAVE_BYTES = {1: (32 * 29 * 4 + 15) // 16 * 16 + 5 * 32 * 16, 2: (64 * 29 * 4 + 15) // 16 * 16 + 5 * 64 * 16}
NETWORK_BYTES = 40 * 1024  # any image size: both plans take it from the same PolicyLds member
TABLE_BYTES = 4096


def _call(fn, n, cus, f16):
    lds = (C.c_ulonglong * 6)(10 ** 9, 10 ** 9, NETWORK_BYTES, TABLE_BYTES, WAVE_BYTES[1], WAVE_BYTES[2])  # no roles shape fits
    o = (C.c_longlong * 6)()
    fn(n, cus, 1 if f16 else 0, lds, o)
    return dict(zip(("status", "kernel", "lds_bytes", "tiles", "n_waves", "workgroups"), o))


@pytest.mark.parametrize("cus", [256, 8])
@pytest.mark.parametrize("f16", [True, False], ids=["f16x3", "f32"])
def test_preview_entry_has_the_plain_kernels_shape(plan, cus, f16):
    edge = 256 * cus
    for n in (1, edge, edge + 1):
        got, want = _call(plan.preview, n, cus, f16), _call(plan.plain, n, cus, f16)
        assert got == want, (n, got, want)
        assert got["status"] == 0 and got["kernel"] == 2  # PolicyKernel::Plain
        small = n <= edge
        tiles = 1 if (f16 and small) else 2
        n_waves = 4 if (not f16 and small) else 8
        assert (got["tiles"], got["n_waves"]) == (tiles, n_waves), n
        assert got["lds_bytes"] == NETWORK_BYTES + TABLE_BYTES + n_waves * WAVE_BYTES[tiles], n
        assert got["workgroups"] == -(-n // (32 * tiles * n_waves)), n


def test_preview_launch_is_planned_by_plan_policy_plain():
    text = open(os.path.join(CSRC, "mse_lib.hip")).read()
    body = re.search(r"static PolicyPlan plan_rollout_policy_preview\(.*?\n\}", text, re.S).group(0)
    assert re.search(r"plan_policy_plain\(h->P\.n, h->cus, pol->use_f16\(\), 1, policy_lds<3>\(h->P\)\)", body), body
    # the launch and the check both ask that function, and there is no other plan for the entry
    assert len(re.findall(r"plan_rollout_policy_preview\(h, pol\)", text)) == 2
    launch = re.search(r"static void launch_rollout_policy_preview\(.*?\n\}", text, re.S).group(0)
    assert "plan.workgroups" in launch and "64 * plan.n_waves" in launch and "plan.lds_bytes" in launch
