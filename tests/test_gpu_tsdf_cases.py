"""The volumetric fusion on the device on the cases of tests/tsdf_cases.py,
whose tallies tests/test_tsdf_cases_cpu.py proves: fields whose cells take all
254 configurations, depths that meet the comparisons of steps 2-8 with
equality, images of 1 to 4 channels, grids that end on and one voxel behind a
brick face, and one case that crosses a tile of the shared scan.  For each:
smvs_tsdf_fuse equals tests/tsdf_ref.py in every array; smvs_tsdf_fuse_sparse
equals tests/tsdf_sparse_ref.py and, up to order, the dense entry; with the
brick cull it equals itself without, no seed brick is culled and
brick_candidate is tests/tsdf_cull_ref.py's.  Every comparison is for
equality of the bits."""
import numpy as np
import pytest

import mesh_clean_ref  # tests/mesh_clean_ref.py
import tsdf_cases as tc  # tests/tsdf_cases.py
import tsdf_cull_ref  # tests/tsdf_cull_ref.py
import tsdf_ref  # tests/tsdf_ref.py
import tsdf_sparse_ref  # tests/tsdf_sparse_ref.py
from test_gpu_tsdf_sparse import _against_dense

pytestmark = pytest.mark.gpu

MESH_KEYS = ("xyz", "normals", "rgb", "confidence", "faces")
DENSE_KEYS = ("weight",) + MESH_KEYS
SPARSE_KEYS = ("brick_state", "weight") + MESH_KEYS + ("cells",)
SPARSE_STATS = ("bricks", "seed_bricks", "allocated_bricks", "state_bytes")


@pytest.fixture(scope="module")
def hip():
    import smvs_amd
    if smvs_amd.device_count() < 1:
        pytest.fail("no HIP device")
    return smvs_amd


def _maps(request, c):
    """the maps the field reads: the oracle's cut maps for the cut case"""
    if not c.cut:
        return c.depths
    oracle = request.getfixturevalue("oracle")
    return oracle.cut_depth_maps(c.cams, c.depths, c.normals)[0]


def _want(request, c, sparse):
    if not c.cut:
        return tc.restated(c.name, sparse)
    ref = tsdf_sparse_ref if sparse else tsdf_ref
    origin, voxel, dims = c.box
    return ref.fuse(c.cams, _maps(request, c), c.images, origin, voxel, dims, **c.kw)


def _args(c):
    origin, voxel, dims = c.box
    return (c.cams, c.depths, c.normals if c.cut else None, c.images, origin, voxel, dims)


def _equal(got, want, keys, label):
    for k in keys:
        assert got[k].shape == want[k].shape, (label, k, got[k].shape, want[k].shape)
        assert got[k].dtype == want[k].dtype, (label, k)
        assert np.array_equal(got[k], want[k]), (label, k)


def _volume_equal(got, want, label):
    assert np.array_equal(np.isnan(got["tsdf"]), np.isnan(want["tsdf"])), label
    assert np.array_equal(got["tsdf"], want["tsdf"], equal_nan=True), label


def _dense(hip, request, name):
    c = tc.get(name)
    got = hip.fuse_tsdf(*_args(c), cut=c.cut, volume=True, **c.kw)
    want = _want(request, c, False)
    print("TSDF-CASES %s voxels=%d unknown=%d vertices=%d faces=%d (device %d, %d)"
          % (name, want["tsdf"].size, np.isnan(want["tsdf"]).sum(), len(want["xyz"]),
             len(want["faces"]), len(got["xyz"]), len(got["faces"])))
    if c.cut:
        s = tc.tally_surface(want["tsdf"])
        print("TSDF-CASES %s (cut) configurations=%d m=%s max faces per edge=%d"
              % (name, len(s["configs"]), sorted(s["m"]), s["max_faces_per_edge"]))
    _volume_equal(got, want, name)
    _equal(got, want, DENSE_KEYS, name)
    assert set(got) == set(want)
    return got


def _sparse(hip, request, name):
    c = tc.get(name)
    got = hip.fuse_tsdf(*_args(c), cut=c.cut, volume=True, sparse=True, brick_state=True, **c.kw)
    want = _want(request, c, True)
    st = want["stats"]
    print("TSDF-CASES sparse %s bricks=%d seed=%d allocated=%d vertices=%d faces=%d (device %d, %d)"
          % (name, st["bricks"], st["seed_bricks"], st["allocated_bricks"], len(want["xyz"]),
             len(want["faces"]), len(got["xyz"]), len(got["faces"])))
    _volume_equal(got, want, name)
    _equal(got, want, SPARSE_KEYS, name)
    assert got["stats"] == st
    assert set(got) == set(want)
    _against_dense(hip, got, c.cams, c.depths, c.normals if c.cut else None, c.images, c.box,
                   c.cut, name, **c.kw)
    return got


def _culled(hip, request, name):
    c = tc.get(name)
    origin, voxel, dims = c.box
    got = hip.fuse_tsdf(*_args(c), cut=c.cut, volume=True, sparse=True, brick_state=True,
                        cull=True, brick_candidate=True, **c.kw)
    plain = hip.fuse_tsdf(*_args(c), cut=c.cut, volume=True, sparse=True, brick_state=True,
                          **c.kw)
    cand = tsdf_cull_ref.candidates(c.cams, _maps(request, c), origin, voxel, dims,
                                    c.kw["trunc"])
    st = got["stats"]
    print("TSDF-CASES cull %s bricks=%d seed=%d allocated=%d tested=%d (restatement %d)"
          % (name, st["bricks"], st["seed_bricks"], st["allocated_bricks"], st["tested_bricks"],
             int(cand.sum())))
    assert set(got) == set(plain) | {"brick_candidate"}
    _volume_equal(got, plain, name)
    _equal(got, plain, SPARSE_KEYS, name)
    assert {k: st[k] for k in SPARSE_STATS} == plain["stats"]
    assert got["brick_candidate"].dtype == np.uint8
    assert np.array_equal(got["brick_candidate"], cand), name
    assert st["tested_bricks"] == int(cand.sum())
    # no seed brick is culled
    assert np.all((got["brick_state"] == 2) <= (got["brick_candidate"] != 0)), name
    return got


@pytest.mark.parametrize("name", tc.SMALL_NAMES)
def test_dense_entry_is_the_restatement(hip, request, name):
    got = _dense(hip, request, name)
    if not tc.get(name).cut:        # (the cut leaves hardly a complete cell)
        assert len(got["faces"]) > 0 and got["faces"].max() < len(got["xyz"])


@pytest.mark.parametrize("name", tc.SMALL_NAMES)
def test_sparse_entry_is_the_restatement_and_the_dense_entry(hip, request, name):
    got = _sparse(hip, request, name)
    assert 0 < got["stats"]["seed_bricks"] <= got["stats"]["allocated_bricks"]


@pytest.mark.parametrize("name", tc.SMALL_NAMES)
def test_culled_sparse_entry_is_the_sparse_entry(hip, request, name):
    got = _culled(hip, request, name)
    assert 0 < got["stats"]["seed_bricks"] <= got["stats"]["tested_bricks"]


def test_exact_case_on_the_device_has_the_zero_value_and_the_equalities(hip):
    """what the CPU test proves of the restatement, read off the device's volume"""
    c = tc.get("exact")
    got = hip.fuse_tsdf(*_args(c), cut=False, volume=True, **c.kw)
    k, j, i = tc.exact_f0_voxel(c)
    assert got["tsdf"][k, j, i] == 0 and got["weight"][k, j, i] == 3
    assert not np.signbit(got["tsdf"][k, j, i])
    # the layer on the cameras' plane is unknown, the one behind it known
    assert np.isnan(got["tsdf"][0]).all() and not np.isnan(got["tsdf"][1]).all()


# ------------------------------------------------- the case that crosses a tile
def test_tiles_dense(hip, request):
    got = _dense(hip, request, "tiles")
    assert got["tsdf"].size > tc.SCAN_TILE * tc.POINT_BLOCK
    assert len(got["xyz"]) > 1 << 16 and len(got["faces"]) > 1 << 16


def test_tiles_sparse(hip, request):
    got = _sparse(hip, request, "tiles")
    assert got["stats"]["allocated_bricks"] > tc.SCAN_TILE


def test_tiles_culled(hip, request):
    got = _culled(hip, request, "tiles")
    assert got["stats"]["allocated_bricks"] > tc.SCAN_TILE
    assert got["stats"]["tested_bricks"] <= got["stats"]["bricks"]


# ------------------------------------------------------------- the mesh clean
CLEAN_CASE = "rough-odd-3v"
CLEAN_COMPONENT = 12


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_clean_of_a_rough_mesh_is_the_restatement(hip, sparse):
    """a fused mesh with edges that four faces share, a threshold (the median
    confidence, a fact of the input) and a component size that both remove
    something"""
    c = tc.get(CLEAN_CASE)
    got = hip.fuse_tsdf(*_args(c), cut=False, sparse=sparse, **c.kw)
    want = tc.restated(CLEAN_CASE, sparse)
    keys = MESH_KEYS + (("cells",) if sparse else ())
    _equal(got, want, keys, CLEAN_CASE)
    mesh = {k: got[k] for k in keys}
    assert tc.tally_surface(tc.field_of(CLEAN_CASE)[0])["max_faces_per_edge"] == 4
    threshold = float(np.median(want["confidence"]))
    opts = dict(threshold=threshold, component_size=CLEAN_COMPONENT)
    expect = mesh_clean_ref.clean(mesh, **opts)
    st = expect["stats"]
    print("TSDF-CASES clean %s n=%d m=%d -> n=%d m=%d %s" % (
        "sparse" if sparse else "dense", len(mesh["xyz"]), len(mesh["faces"]),
        len(expect["xyz"]), len(expect["faces"]), st))
    assert st["n_cut"] > 0 and st["n_small_components"] > 0 and st["n_small_vertices"] > 0
    assert 0 < len(expect["faces"]) < len(mesh["faces"])
    cleaned = hip.clean_mesh(mesh, labels=True, **opts)
    mesh_clean_ref.assert_same(cleaned, expect, cells=sparse)
