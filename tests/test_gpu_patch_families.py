"""Scale 6 (16 x 16 samples per patch, four chunks of 64): the default form of
the patch kernel, gn_patch_kernel<1, 4> -- phase 1 of the four chunks on four
waves, then every wave walking ONE accumulator chain (an MFMA block family or
the gradient sum) through all four chunks in chunk order -- against one wave
walking the chunks one after the other (SMVS_PATCH_SPLIT=0): the same bits in
every patch system and the same Newton loop.

The switch is read once per process, so each side is one child process; it
runs every case and the tests compare what the two children left.

Shapes: synth.make_problem(256, 192, n_subs, 6) is a 2 x 1 patch grid (3 x 2
nodes), the smallest the scale has: a launch of eight workgroups of which two
(all nodes active) or one (partial set) find a patch.
  n_subs = 1: the LDS region of a chunk is the 27-row minimum, nothing larger
              is aliased with the pixel systems the other waves read;
  n_subs = 8: 35 rows, the aliased neighbour scratch is the larger one.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WIDTH, HEIGHT, SCALE = 256, 192, 6
NEIGHBOURS = (1, 8)
ACTIVE_SETS = ("all", "partial")
REG, LIGHT_REG = 0.01, 0.5

_PROBE = r"""
import json, sys
import numpy as np
import torch  # noqa: F401  (one HIP runtime, see conftest.py)
sys.path.insert(0, sys.argv[1])
import smvs_amd
from smvs_amd import synth
systems, stats = {}, {}
for n_subs in (1, 8):
    for shading in (False, True):
        prob = synth.make_problem(256, 192, n_subs, 6, shading=shading)
        surf = prob["surf"]
        lit = dict(light_reg=0.5, lighting=prob["lighting"]) if shading else {}
        ctx = smvs_amd.ViewContext(256, 192, n_subs)
        ctx.set_views(prob["views"])
        # (all nodes first: whatever the partial run leaves untouched in the
        # patch records is then this run's, not fresh memory)
        for case in ("all", "partial"):
            active = np.load(sys.argv[3])[case] & surf["node_valid"]
            ctx.set_surface(surf)
            ctx.set_active(active)
            ctx.gn_construct(0.01, **lit)
            Hp, gp = ctx.gn_patch_systems()
            key = "%d-%s-%s" % (n_subs, case, "shaded" if shading else "plain")
            systems[key] = np.concatenate([Hp.reshape(len(Hp), -1), gp.reshape(len(gp), -1)], 1)
            st = ctx.run_loop(0.01, max_newton_steps=3, reset_active=False, **lit)
            stats[key] = {k: int(v) for k, v in st.items()}
        ctx.close()
np.savez(sys.argv[2], **systems)
print(json.dumps(stats))
"""


def _grid():
    from smvs_amd import synth
    return synth.grid_for_scale(WIDTH, HEIGHT, SCALE)


def _active_sets():
    """Node flags of the two cases: every node, and the last node column
    alone -- the patches of the last patch column are live, no other."""
    g = _grid()
    rows, stride = g["npy"] + 1, g["npx"] + 1
    partial = np.zeros((rows, stride), np.uint8)
    partial[:, stride - 1] = 1
    return dict(all=np.ones(rows * stride, np.uint8), partial=partial.reshape(-1))


def _live_patches(active):
    g = _grid()
    a = active.reshape(g["npy"] + 1, g["npx"] + 1)
    return (a[:-1, :-1] | a[:-1, 1:] | a[1:, :-1] | a[1:, 1:]).reshape(-1) != 0


@pytest.fixture(scope="module")
def sides(tmp_path_factory):
    import smvs_amd
    if smvs_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on a GPU")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tmp = tmp_path_factory.mktemp("patch_families")
    np.savez(str(tmp / "active.npz"), **_active_sets())
    out = {}
    for tag, extra in (("families", {}), ("serial", {"SMVS_PATCH_SPLIT": "0"})):
        env = dict(os.environ, **extra)
        res = subprocess.run([sys.executable, "-c", _PROBE, root, str(tmp / (tag + ".npz")),
                              str(tmp / "active.npz")],
                             env=env, capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stderr[-2000:]
        with np.load(str(tmp / (tag + ".npz"))) as z:
            systems = {k: z[k] for k in z.files}
        out[tag] = (systems, json.loads(res.stdout.strip().splitlines()[-1]))
    return out


def test_cases_are_what_they_claim():
    """All nodes: every patch is live; partial: a live list shorter than the
    launch (rounded up to eight workgroups), the last band of eight partly
    empty -- the surplus workgroups leave."""
    from smvs_amd import synth
    sets = _active_sets()
    for n_subs in NEIGHBOURS:
        surf = synth.make_problem(WIDTH, HEIGHT, n_subs, SCALE)["surf"]
        # (a patch of 64 pixels sampled every 4th: 16 x 16 = four chunks of 64)
        assert ((1 << SCALE) // 4) ** 2 == 4 * 64
        valid = surf["patch_valid"] != 0
        assert valid.all() and valid.size >= 2
        live_all = _live_patches(sets["all"] & surf["node_valid"]) & valid
        live_part = _live_patches(sets["partial"] & surf["node_valid"]) & valid
        assert live_all.all()
        assert 0 < live_part.sum() < live_all.sum() and live_part.sum() % 8 != 0


@pytest.mark.parametrize("shading", ["plain", "shaded"])
@pytest.mark.parametrize("case", ACTIVE_SETS)
@pytest.mark.parametrize("n_subs", NEIGHBOURS)
def test_family_waves_equal_one_wave(sides, n_subs, case, shading):
    key = "%d-%s-%s" % (n_subs, case, shading)
    got, got_stats = sides["families"]
    want, want_stats = sides["serial"]
    assert got[key].shape == want[key].shape
    live = _live_patches(_active_sets()[case])
    # (every live patch has a system: the comparison is not of zeros)
    assert live.any() and np.abs(want[key][live]).max(axis=1).min() > 0
    assert np.abs(want[key]).max() > 0
    assert np.array_equal(got[key], want[key])
    assert got_stats[key] == want_stats[key]
    assert got_stats[key]["newton_steps"] >= 1 and got_stats[key]["nan_break"] == 0
