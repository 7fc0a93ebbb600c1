"""Which form of the SGM path aggregation a run takes (smvs_amd/csrc/sgm_path_plan.h)
on the CPU: plain host arithmetic, built here with g++ behind a small extern "C"
shim.  The plan picks the kernel family, its template arguments, whether S is
zeroed first, the WTA kernel that follows and what the workspace holds, so every
field is compared with a transcription of the rule written here, over every plane
count the entries admit."""
import ctypes as C
import os
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "smvs_amd", "csrc")
WIDE, PAIRS, LINES, PER_DIRECTION = "WIDE", "PAIRS", "LINES", "PER_DIRECTION"
SUM_WIDE, SUM, ROWS = "sum-wide", "sum", "rows"

# every admitted plane count: 2 ... 128 and the multiples of 8 from 136 to 256
PLANES = list(range(2, 129)) + list(range(136, 257, 8))
# the default, the last that fits a byte, the first that does not, the largest
# check_sgm_penalties admits (8 (255 + P) + 4 * 255 < 65536)
PENALTIES = [96, 255, 256, 7808]

SHIM = r"""
#include "sgm_path_plan.h"
using namespace smvs_hip;
extern "C" void
path_plan(int num_steps, unsigned largest_p2, int wave_per_line, int *out)
{
    SgmPathPlan const p = sgm_path_plan(num_steps, largest_p2, wave_per_line != 0);
    out[0] = p.form == SGM_PATHS_WIDE ? 0 : p.form == SGM_PATHS_PAIRS ? 1
        : p.form == SGM_PATHS_LINES ? 2 : p.form == SGM_PATHS_PER_DIRECTION ? 3 : -1;
    out[1] = p.delta;
    out[2] = p.full;
    out[3] = p.zero_s;
    out[4] = p.wta == SGM_WTA_SUM_WIDE ? 0 : p.wta == SGM_WTA_SUM ? 1
        : p.wta == SGM_WTA_ROWS ? 2 : -1;
    out[5] = p.needs_s(false);
    out[6] = p.needs_s(true);
}
"""


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    d = tmp_path_factory.mktemp("sgm_path_plan")
    shim = d / "shim.cc"
    shim.write_text(SHIM)
    out = str(d / "libsgm_path_plan_test.so")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared",
                           "-I", CSRC, "-o", out, str(shim)])
    lib = C.CDLL(out)
    lib.path_plan.restype = None
    lib.path_plan.argtypes = [C.c_int, C.c_uint, C.c_int, C.POINTER(C.c_int)]

    def call(num_steps, largest_p2, wave_per_line=False):
        buf = (C.c_int * 7)()
        lib.path_plan(num_steps, largest_p2, int(wave_per_line), buf)
        return dict(form=(WIDE, PAIRS, LINES, PER_DIRECTION)[buf[0]], delta=bool(buf[1]),
                    full=bool(buf[2]), zero_s=bool(buf[3]), wta=(SUM_WIDE, SUM, ROWS)[buf[4]],
                    s_volume=bool(buf[5]), s_volume_wanted=bool(buf[6]))
    return call


def expected(num_steps, largest_p2, wave_per_line):
    """The rule, transcribed."""
    delta = num_steps % 4 == 0 and largest_p2 <= 255
    full = zero_s = False
    if num_steps > 128:
        form, full, zero_s = WIDE, num_steps == 256, not delta
    elif delta and not wave_per_line:
        form, full = PAIRS, num_steps == 128
    elif delta:
        form = LINES
    elif num_steps % 2 == 0:
        form, zero_s = LINES, True
    else:
        form = PER_DIRECTION
    wta = (SUM_WIDE if num_steps > 128 else SUM) if delta else ROWS
    # the workspace: S only when the paths write it or the caller wants it
    return dict(form=form, delta=delta, full=full, zero_s=zero_s, wta=wta,
                s_volume=not delta, s_volume_wanted=True)


def test_every_field_follows_the_rule(plan):
    seen = set()
    for num_steps in PLANES:
        for p2 in PENALTIES:
            for wave_per_line in (False, True):
                got = plan(num_steps, p2, wave_per_line)
                assert got == expected(num_steps, p2, wave_per_line), (num_steps, p2, wave_per_line)
                # what the kernels rely on: bytes are read and written as u32 and
                # summed by the sum kernels; atomics need a zeroed S and u16 pairs
                if got["delta"]:
                    assert num_steps % 4 == 0 and p2 <= 255 and not got["zero_s"]
                    assert got["wta"] in (SUM_WIDE, SUM)
                else:
                    assert got["wta"] == ROWS and got["s_volume"]
                if got["zero_s"]:
                    assert num_steps % 2 == 0 and got["form"] in (WIDE, LINES)
                if got["form"] == PAIRS:
                    assert got["delta"] and num_steps <= 128
                if got["form"] != WIDE:
                    assert num_steps <= 128
                seen.add((got["form"], got["delta"], got["full"]))
    # every kernel family in every form the launcher can instantiate
    assert seen == {(WIDE, True, True), (WIDE, True, False), (WIDE, False, True),
                    (WIDE, False, False), (PAIRS, True, True), (PAIRS, True, False),
                    (LINES, True, False), (LINES, False, False), (PER_DIRECTION, False, False)}


def test_named_edges(plan):
    p = plan(128, 96)
    assert (p["form"], p["full"], p["delta"], p["wta"]) == (PAIRS, True, True, SUM)
    p = plan(136, 96)
    assert (p["form"], p["full"], p["delta"], p["wta"]) == (WIDE, False, True, SUM_WIDE)
    p = plan(256, 96)
    assert (p["form"], p["full"], p["delta"], p["wta"]) == (WIDE, True, True, SUM_WIDE)
    # 255 against 256 flips delta, zero_s and the WTA kernel
    for num_steps in (136, 256):
        a, b = plan(num_steps, 255), plan(num_steps, 256)
        assert (a["delta"], a["zero_s"], a["wta"]) == (True, False, SUM_WIDE)
        assert (b["delta"], b["zero_s"], b["wta"]) == (False, True, ROWS)
        assert a["form"] == b["form"] == WIDE and a["full"] == b["full"]
    a, b = plan(128, 255), plan(128, 256)
    assert (a["form"], a["delta"], a["zero_s"], a["wta"]) == (PAIRS, True, False, SUM)
    assert (b["form"], b["delta"], b["zero_s"], b["wta"]) == (LINES, False, True, ROWS)
    # a wave per line is an option up to 128 planes only
    assert plan(128, 96, wave_per_line=True)["form"] == LINES
    assert plan(128, 96, wave_per_line=True)["delta"] and not plan(128, 96, True)["zero_s"]
    for num_steps in (136, 200, 256):
        for p2 in PENALTIES:
            assert plan(num_steps, p2, True) == plan(num_steps, p2, False)
    # planes in twos, not in fours: u16 pairs with atomics
    p = plan(62, 96)
    assert (p["form"], p["delta"], p["zero_s"], p["wta"]) == (LINES, False, True, ROWS)
    # an odd count: a launch per direction, the first of which writes S
    p = plan(37, 96)
    assert (p["form"], p["delta"], p["zero_s"], p["full"], p["wta"]) \
        == (PER_DIRECTION, False, False, False, ROWS)


def test_workspace_volumes(plan):
    """delta <=> the eight path-byte volumes (SgmWorkspace::ensure asks for them
    on plan.delta); S only when not delta or when the caller wants it."""
    for num_steps in PLANES:
        for p2 in PENALTIES:
            p = plan(num_steps, p2)
            assert p["s_volume"] == (not p["delta"])
            assert p["s_volume_wanted"]
