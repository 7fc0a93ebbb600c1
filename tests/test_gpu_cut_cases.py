"""smvs_cut_depth_maps on the view sets of tests/cut_cases.py, where every
branch of mesh_cut_kernel decides (test_cut_cases_cpu.py holds the tallies):
the cut maps and world normals equal to the oracle's, view by view, to the bit;
and every export that reads the cut -- points, mesh, simplified, dense and
sparse TSDF fusion -- on the views of mixed size and of degenerate size,
against its own restatement run on the oracle's cut maps, with the comparisons
of its own test file (array_equal; recalc_normals within 1e-6)."""
import numpy as np
import pytest

import cut_cases as cc  # tests/cut_cases.py
import cut_ref  # tests/cut_ref.py
import mesh_ref  # tests/mesh_ref.py
import points_ref  # tests/points_ref.py
import simplify_ref  # tests/simplify_ref.py
import tsdf_ref  # tests/tsdf_ref.py
from test_gpu_mesh import _assert_same as assert_same_mesh
from test_gpu_points import _assert_same as assert_same_points
from test_gpu_simplify import _assert_same_export as assert_same_simplified
from test_gpu_simplify import _cut_maps
from test_gpu_tsdf import _compare as compare_tsdf
from test_gpu_tsdf_sparse import _against_restatement as compare_tsdf_sparse

pytestmark = pytest.mark.gpu

EXPORT_SETS = ("mixed_wide", "degenerate_sizes")
VOXELS_PER_SIDE = 40


@pytest.fixture(scope="module")
def hip():
    import smvs_amd
    if smvs_amd.device_count() < 1:
        pytest.fail("no HIP device")
    return smvs_amd


def _first_difference(name, i, got, want):
    """None, or the message for the first pixel of view i that differs: the
    view, the pixel, both values and what the restatement did there."""
    bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    if len(bad) == 0:
        return None
    y, x = int(bad[0][0]), int(bad[0][1])
    return "%s view %d pixel (x %d, y %d)%s: device %r oracle %r (%d pixels differ); %s" % (
        name, i, x, y, "" if got.ndim == 2 else " channel %d" % bad[0][2], got[tuple(bad[0])],
        want[tuple(bad[0])], len(bad), cut_ref.describe(cc.restated(name)[2][i], y, x))


@pytest.mark.parametrize("name", cc.NAMES)
def test_cut_matches_oracle_view_by_view(hip, oracle, name):
    """Each view's cut map against the oracle run on the same list in the same
    order (mixed_wide and its reverse are two cases: the float sum depends on
    the order, so nothing is asserted across them)."""
    c = cc.get(name)
    want_d, want_n = cc.oracle_cut(oracle, name)
    got_d, got_n = hip.cut_depth_maps(c.cams, c.depths, c.normals)
    assert len(got_d) == len(want_d) == len(c.cams)
    for i in range(len(c.cams)):
        assert got_d[i].shape == want_d[i].shape and got_n[i].shape == want_n[i].shape
        message = _first_difference(name, i, got_n[i], want_n[i])
        assert message is None, "world normals: " + message
        message = _first_difference(name, i, got_d[i], want_d[i])
        assert message is None, "cut map: " + message


def _set(name, simplified=False):
    """The views of an export set; for the simplified export without the view
    that smvs_simplify_triangulate refuses (fewer than 2 x 2 pixels)."""
    c = cc.get(name)
    keep = [i for i, d in enumerate(c.depths) if not simplified or min(d.shape) >= 2]
    return [[part[i] for i in keep] for part in (c.cams, c.depths, c.normals, c.images)]


@pytest.mark.parametrize("cut", [True, False])
@pytest.mark.parametrize("name", EXPORT_SETS)
def test_points(hip, oracle, name, cut):
    cams, depths, normals, images = _set(name)
    got = hip.generate_points(cams, depths, normals, images, cut=cut, faces=True, cut_maps=True)
    dms, wn = _cut_maps(oracle, cams, depths, normals, cut)
    for a, b in zip(got["cut_depth"], dms):
        assert np.array_equal(a, b)
    assert_same_points(got, points_ref.points(cams, dms, wn, images))


@pytest.mark.parametrize("cut", [True, False])
@pytest.mark.parametrize("name", EXPORT_SETS)
def test_mesh(hip, oracle, name, cut):
    cams, depths, normals, images = _set(name)
    got = hip.generate_mesh(cams, depths, normals, images, cut=cut)
    dms, wn = _cut_maps(oracle, cams, depths, normals, cut)
    assert_same_mesh(got, mesh_ref.mesh(cams, dms, wn, images), "%s-cut%d" % (name, cut))


@pytest.mark.parametrize("mesh", [False, True])
@pytest.mark.parametrize("cut", [True, False])
@pytest.mark.parametrize("name", EXPORT_SETS)
def test_simplified(hip, oracle, name, cut, mesh):
    from smvs_amd._capi import SmvsError
    cams, depths, normals, images = _set(name, simplified=True)
    refused = [d for d in cc.get(name).depths if min(d.shape) < 2]
    assert len(refused) == (name == "degenerate_sizes")
    for d in refused:       # a one-column map: refused alone and within a set
        with pytest.raises(SmvsError):
            hip.simplify_triangulate(d)
        with pytest.raises(SmvsError):
            hip.generate_simplified(*_set(name), mesh=mesh, cut=cut)
    got = hip.generate_simplified(cams, depths, normals, images, mesh=mesh, cut=cut)
    dms, wn = _cut_maps(oracle, cams, depths, normals, cut)
    want = simplify_ref.simplified(cams, dms, wn, images, mesh=mesh)
    assert_same_simplified(got, want, mesh, "%s-cut%d-mesh%d" % (name, cut, mesh))


def _box(oracle, name):
    """About 40 voxels along the longest side of the box of the cut maps'
    world points."""
    c = cc.get(name)
    lo, hi = tsdf_ref.bounds(c.cams, cc.oracle_cut(oracle, name)[0])
    voxel = float((hi - lo).max()) / VOXELS_PER_SIDE
    dims = tuple(int(n) for n in np.maximum(np.ceil((hi - lo) / voxel), 2).astype(int) + 1)
    assert max(dims) <= VOXELS_PER_SIDE + 2
    return tuple(float(v) for v in lo - 0.5 * voxel), voxel, dims


@pytest.mark.parametrize("cut", [True, False])
@pytest.mark.parametrize("name", EXPORT_SETS)
def test_tsdf_dense(hip, oracle, name, cut):
    cams, depths, normals, images = _set(name)
    origin, voxel, dims = _box(oracle, name)
    got = compare_tsdf(hip, oracle, cams, depths, normals, images, origin, voxel, dims, cut,
                       "%s-cut%d" % (name, cut))
    assert len(got["faces"]) > 0


@pytest.mark.parametrize("cut", [True, False])
@pytest.mark.parametrize("name", EXPORT_SETS)
def test_tsdf_sparse(hip, oracle, name, cut):
    cams, depths, normals, images = _set(name)
    got = compare_tsdf_sparse(hip, oracle, cams, depths, normals, images, _box(oracle, name),
                              cut, "%s-cut%d" % (name, cut))
    assert len(got["faces"]) > 0
