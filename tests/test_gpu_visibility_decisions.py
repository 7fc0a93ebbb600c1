"""topo_visibility_kernel (csrc/topo_visibility.hip) on inputs where its last
two tests decide: the warp anisotropy (`worst > 8`) and ncc_for_patch -- the
"all samples inside" check, the norm test, `ncc < 0` -- against the CPU oracle's
masks (orc_topology_subviews, depth_optimizer.cc:433-604, 792-912 transcribed)
on tests/visibility_cases.py, array_equal throughout.

On synth's renderings (test_gpu_parity.py's topology tests) the NCC is far
above zero and decides almost nothing; here the images are independent noise,
its sign is a coin flip per pair, and a wrong tap, weight, channel, mean or
reduction moves many mask bits.  tests/test_visibility_cases_cpu.py shows
without a GPU that every case decides what it is here for and that no decision
sits within 1e-9 of its threshold, so the order of the device's sums cannot
flip one.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import visibility_cases as vc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import smvs_amd
    if smvs_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on a GPU")
    return smvs_amd


SWITCHES = ("SMVS_NCC_PAIRS", "SMVS_TOPO_DIVIDE", "SMVS_ZBUF_WINDOW")


def _context(hip, case, k):
    """A context with the cameras, image set k (its own scale space) and the
    all-valid surface of a case."""
    g = vc.geometry(case)
    ctx = hip.ViewContext(case.w, case.h, case.n_subs)
    ctx.set_views(g["views"])                     # cameras (the planes are replaced below)
    for v, img in enumerate(vc.images(case, k)):
        ctx.upload_image(v - 1, img)
    ctx.set_scale(case.scale)
    ctx.set_surface(g["surf"])
    return ctx


def _differences(got, want, n_subs):
    bits = (got ^ want)[:, None] >> np.arange(n_subs, dtype=np.uint32) & 1
    return "%d mask bits differ (patch, neighbour): %s" % (
        bits.sum(), np.argwhere(bits)[:8].tolist())


@pytest.mark.parametrize("case", vc.CASES, ids=vc.ids(vc.CASES))
def test_visibility_masks_match_the_oracle_where_ncc_and_anisotropy_decide(hip, oracle, case):
    for k in range(case.sets):
        want = vc.oracle_mask(oracle, case, k)
        ctx = _context(hip, case, k)
        try:
            got = ctx.topology_subviews(None, use_ncc=True)
        finally:
            ctx.close()
        assert np.array_equal(got, want), (k, _differences(got, want, case.n_subs))


@pytest.mark.parametrize("case", vc.NOISE[1:], ids=vc.ids(vc.NOISE[1:]))
def test_noise_masks_under_every_switch_of_the_kernel(hip, oracle, monkeypatch, case):
    """The kernel's other forms on masks the NCC did decide: its samples one at
    a time instead of in pairs (SMVS_NCC_PAIRS=0 -- RGB views, so the pairs are
    what the default runs), every quotient a division (SMVS_TOPO_DIVIDE=exact),
    the z-buffer as the reference keeps it (SMVS_ZBUF_WINDOW=3), and 1 to 256
    lanes per (patch, neighbour) (SMVS_VIS_GROUP_<ps>): DPP rows, permlane
    swaps and LDS across waves sum in another order, other samples go to the
    LDS stash, and one lane per pair from patch size 16 on has more samples than
    its registers and the stash hold -- the recompute branch."""
    group = "SMVS_VIS_GROUP_%d" % (1 << case.scale)
    modes = [("SMVS_NCC_PAIRS", "0"), ("SMVS_TOPO_DIVIDE", "exact"), ("SMVS_ZBUF_WINDOW", "3")]
    modes += [(group, str(lanes)) for lanes in (1, 2, 16, 32, 64, 256)]
    for name in SWITCHES + (group,):
        monkeypatch.delenv(name, raising=False)
    surf = vc.geometry(case)["surf"]
    for k in range(case.sets):
        want = vc.oracle_mask(oracle, case, k)
        ctx = _context(hip, case, k)
        try:
            for name, value in modes:
                monkeypatch.setenv(name, value)
                ctx.set_surface(surf)
                got = ctx.topology_subviews(None, use_ncc=True)
                monkeypatch.delenv(name)
                assert np.array_equal(got, want), (k, name, value,
                                                   _differences(got, want, case.n_subs))
        finally:
            ctx.close()


def test_noise_masks_without_the_lds_stash(hip, oracle, tmp_path):
    """SMVS_NCC_STASH=0 (read once per process, hence a fresh child): the
    samples a lane does not keep in registers are warped and interpolated again
    in the second pass instead of being read back from LDS.  Scales 3 to 6,
    where a lane has more samples than it keeps."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cases = [c for c in vc.NOISE if c.scale >= 3]
    probe = r"""
import json, os, sys
import numpy as np
import torch  # noqa: F401  (one HIP runtime, see conftest.py)
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import smvs_amd
import visibility_cases as vc
assert os.environ["SMVS_NCC_STASH"] == "0"
out = {}
for name in sys.argv[3:]:
    case = vc.BY_NAME[name]
    g = vc.geometry(case)
    for k in range(case.sets):
        ctx = smvs_amd.ViewContext(case.w, case.h, case.n_subs)
        ctx.set_views(g["views"])
        for v, img in enumerate(vc.images(case, k)):
            ctx.upload_image(v - 1, img)
        ctx.set_scale(case.scale)
        ctx.set_surface(g["surf"])
        out["%s/%d" % (name, k)] = ctx.topology_subviews(None, use_ncc=True)
        ctx.close()
np.savez(sys.argv[2], **out)
print(json.dumps(sorted(out)))
"""
    path = str(tmp_path / "masks.npz")
    env = dict(os.environ, SMVS_NCC_STASH="0")
    for name in SWITCHES + tuple("SMVS_VIS_GROUP_%d" % (1 << c.scale) for c in cases):
        env.pop(name, None)
    res = subprocess.run([sys.executable, "-c", probe, root, path] + [c.name for c in cases],
                         env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    keys = json.loads(res.stdout.strip().splitlines()[-1])
    masks = np.load(path)
    assert keys == sorted("%s/%d" % (c.name, k) for c in cases for k in range(c.sets))
    for case in cases:
        for k in range(case.sets):
            got, want = masks["%s/%d" % (case.name, k)], vc.oracle_mask(oracle, case, k)
            assert np.array_equal(got, want), (case.name, k,
                                               _differences(got, want, case.n_subs))
