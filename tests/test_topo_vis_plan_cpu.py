"""The launch shape of topo_visibility_kernel (smvs_amd/csrc/topo_vis_plan.h) on
the CPU: plain host arithmetic, built here with g++ behind a small extern "C"
shim.  The shape sizes the dynamic LDS the kernel then indexes, so every output
is compared with a transcription of the rule written here: lanes per (patch,
neighbour) by patch size, the stash slots a lane's samples need beyond the four
it keeps (16 at most), the staged depths and the interior template only while
all of it fits 52 KB -- the depths are dropped first."""
import ctypes as C
import os
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "smvs_amd", "csrc")
BUDGET = 52 * 1024
PATCH_SIZES = [1, 2, 4, 8, 16, 32, 64]
GROUPS = {1: 1, 2: 2, 4: 4, 8: 8, 16: 32, 32: 64, 64: 256}

SHIM = r"""
#include "topo_vis_plan.h"
extern "C" void
vis_shape(int ps, int use_ncc, int n_max, int tpl_n, int group_override, int no_stash,
    long long *out)
{
    smvs_hip::VisLaunchShape const s = smvs_hip::vis_launch_shape(ps, use_ncc != 0, n_max, tpl_n,
        group_override, no_stash != 0);
    out[0] = s.group;
    out[1] = s.ncc_stash_slots;
    out[2] = s.lds_depth_doubles;
    out[3] = s.lds_tpl_n;
    out[4] = (long long)s.dynamic_lds_bytes;
}
"""


@pytest.fixture(scope="module")
def shape(tmp_path_factory):
    d = tmp_path_factory.mktemp("topo_vis_plan")
    shim = d / "shim.cc"
    shim.write_text(SHIM)
    out = str(d / "libtopo_vis_plan_test.so")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared",
                           "-I", CSRC, "-o", out, str(shim)])
    lib = C.CDLL(out)
    lib.vis_shape.restype = None
    lib.vis_shape.argtypes = [C.c_int] * 6 + [C.POINTER(C.c_longlong)]

    def call(ps, use_ncc, n_max, tpl_n, group_override=0, no_stash=False):
        buf = (C.c_longlong * 5)()
        lib.vis_shape(ps, int(use_ncc), n_max, tpl_n, group_override, int(no_stash), buf)
        return dict(zip(("group", "ncc_stash_slots", "lds_depth_doubles", "lds_tpl_n",
                         "dynamic_lds_bytes"), buf))
    return call


def expected(ps, use_ncc, n_max, tpl_n, group_override, no_stash):
    """The rule, transcribed."""
    group = GROUPS[ps]
    g = group_override
    if g == 256 or (1 <= g <= 64 and g & (g - 1) == 0):
        group = g
    if not use_ncc:
        return dict(group=group, ncc_stash_slots=0, lds_depth_doubles=0, lds_tpl_n=0,
                    dynamic_lds_bytes=0)
    per_lane = (n_max + group - 1) // group
    slots = 0 if no_stash else min(16, max(0, per_lane - 4))
    used = slots * 3 * 256 * 4
    depth_doubles = (256 // group) * (ps * ps + 4)
    depths = 0
    if group <= 256 and used + depth_doubles * 8 <= BUDGET:
        depths = depth_doubles
        used += depth_doubles * 8
    tpl = 0
    if used + tpl_n * 8 <= BUDGET:
        tpl = tpl_n
        used += tpl_n * 8
    return dict(group=group, ncc_stash_slots=slots, lds_depth_doubles=depths, lds_tpl_n=tpl,
                dynamic_lds_bytes=used)


@pytest.mark.parametrize("ps", PATCH_SIZES)
def test_lanes_per_pair_by_patch_size(shape, ps):
    for use_ncc in (False, True):
        assert shape(ps, use_ncc, ps * ps + 4 * ps + 4, ps * ps + 4 * ps + 4)["group"] == GROUPS[ps]


@pytest.mark.parametrize("ps", PATCH_SIZES)
def test_group_overrides(shape, ps):
    n = ps * ps + 4 * ps + 4
    for g in (1, 2, 16, 32, 64, 256):
        assert shape(ps, True, n, n, group_override=g)["group"] == g
        assert shape(ps, False, n, n, group_override=g)["group"] == g
    for g in (0, 3, 128, 512):
        assert shape(ps, True, n, n, group_override=g)["group"] == GROUPS[ps]


@pytest.mark.parametrize("ps", PATCH_SIZES)
def test_without_ncc_no_dynamic_lds(shape, ps):
    for g in (0, 1, 64, 256):
        s = shape(ps, False, 5000, 5000, group_override=g)
        assert (s["ncc_stash_slots"], s["lds_depth_doubles"], s["lds_tpl_n"],
                s["dynamic_lds_bytes"]) == (0, 0, 0, 0)


def sweep():
    for ps in PATCH_SIZES:
        pp = ps * ps
        # template lengths around the patch (the border samples make them 2 - 3 x
        # the patch at the fine scales: 44 at patch size 4), then long enough for
        # more than 4 + 16 samples per lane, then too long for the budget
        lengths = sorted({1, pp, pp + 4, pp + 4 * ps + 4, 44, 3 * pp, 5 * GROUPS[ps], 20 * GROUPS[ps],
                          21 * GROUPS[ps], 40 * GROUPS[ps], 2000, 5000, 7000, 20000})
        for n_max in lengths:
            for tpl_n in (0, 1, min(n_max, pp + 4), n_max):
                for g in (0, 1, 8, 64, 256):
                    for no_stash in (False, True):
                        yield ps, n_max, tpl_n, g, no_stash


def test_every_output_follows_the_rule(shape):
    seen_cap = seen_44 = dropped_depths = dropped_tpl = False
    for ps, n_max, tpl_n, g, no_stash in sweep():
        got = shape(ps, True, n_max, tpl_n, group_override=g, no_stash=no_stash)
        want = expected(ps, True, n_max, tpl_n, g, no_stash)
        assert got == want, (ps, n_max, tpl_n, g, no_stash)
        assert got["dynamic_lds_bytes"] <= BUDGET
        assert got["dynamic_lds_bytes"] == got["ncc_stash_slots"] * 3 * 256 * 4 \
            + got["lds_depth_doubles"] * 8 + got["lds_tpl_n"] * 8
        # the depths are dropped before the template is: a template that is left
        # out would not have fitted beside the stash and whatever depths there are
        if got["lds_tpl_n"] == 0 and tpl_n > 0:
            assert got["ncc_stash_slots"] * 3 * 256 * 4 + got["lds_depth_doubles"] * 8 \
                + tpl_n * 8 > BUDGET
            dropped_tpl = True
        if got["lds_depth_doubles"] == 0:
            depth_bytes = (256 // got["group"]) * (ps * ps + 4) * 8
            assert got["ncc_stash_slots"] * 3 * 256 * 4 + depth_bytes > BUDGET
            dropped_depths = dropped_depths or got["lds_tpl_n"] > 0
        seen_cap = seen_cap or got["ncc_stash_slots"] == 16
        if ps == 4 and n_max == 44 and g == 0 and not no_stash:
            # 44 samples over 4 lanes: 11 per lane, 4 kept, 7 in the stash
            assert got["ncc_stash_slots"] == 7
            seen_44 = True
        if no_stash:
            assert got["ncc_stash_slots"] == 0
    assert seen_cap and seen_44 and dropped_depths and dropped_tpl
