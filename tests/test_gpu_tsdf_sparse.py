"""smvs_tsdf_fuse_sparse on the device: equal to the bit, NaN positions
included, to the numpy restatement of its definition (tests/
tsdf_sparse_ref.py on the oracle's cut maps) and, up to the order of vertices
and faces, to the dense device entry smvs_tsdf_fuse; on grids the dense entry
refuses; and through the scene entry."""
import os

import numpy as np
import pytest

import mesh_ref  # tests/mesh_ref.py
import tsdf_sparse_ref  # tests/tsdf_sparse_ref.py

pytestmark = pytest.mark.gpu

MESH_KEYS = ("xyz", "normals", "rgb", "confidence", "faces")
ALL_KEYS = ("brick_state", "weight") + MESH_KEYS + ("cells",)
VOXEL = 0.06
# no side a multiple of a brick side; around the sphere's visible front (z = 3)
SMALL = ((-1.1, -0.9, 2.8), VOXEL, (37, 29, 23))
# reaches toward the cameras: most bricks are not allocated, and free space in
# front of the surface is known to the dense field but not allocated
DEEP = ((-1.22, -1.06, 0.45), 0.04, (61, 53, 75))


@pytest.fixture(scope="module")
def hip():
    import smvs_amd
    if smvs_amd.device_count() < 1:
        pytest.fail("no HIP device")
    return smvs_amd


def _inputs(n_views, w, h, channels, seed=5, last_size=None):
    """The views of test_gpu_tsdf.py (1 % holes, noise, a depth step in view
    0); with last_size the last view has a size of its own."""
    from smvs_amd import synth
    inputs = synth.pipeline_inputs("sphere", w, h, max(n_views - 1, 1), flen=1.2)
    cams = inputs["cams"][:n_views]
    if last_size is not None:
        c = cams[-1]
        cams[-1] = synth.Camera(c.R, c.t, c.flen, last_size[0], last_size[1])
    depths, normals = synth.depth_and_normal_maps(inputs["scene"], cams)
    rng = np.random.default_rng(seed)
    images = []
    for i in range(n_views):
        depths[i] *= (1.0 + 0.002 * rng.standard_normal(depths[i].shape)).astype(np.float32)
        depths[i][rng.random(depths[i].shape) < 0.01] = 0.0          # holes
    depths[0][h // 5:h // 5 + 9, w // 4:w // 4 + 13] *= np.float32(0.8)   # a step
    for d in depths:
        images.append(rng.integers(0, 256, d.shape if channels == 1 else d.shape + (channels,))
                      .astype(np.uint8))
    return cams, depths, normals, images


def _cut_maps(oracle, cams, depths, normals, cut):
    if cut and len(cams) > 1:
        return oracle.cut_depth_maps(cams, depths, normals)[0]
    return depths


def _equal(got, want, keys, label):
    for k in keys:
        assert got[k].shape == want[k].shape, (label, k, got[k].shape, want[k].shape)
        assert got[k].dtype == want[k].dtype, (label, k)
        assert np.array_equal(got[k], want[k]), (label, k)


def _against_restatement(hip, oracle, cams, depths, normals, images, box, cut, label, **kw):
    origin, voxel, dims = box
    got = hip.fuse_tsdf(cams, depths, normals, images, origin, voxel, dims, cut=cut,
                        volume=True, sparse=True, brick_state=True, **kw)
    dms = _cut_maps(oracle, cams, depths, normals, cut)
    want = tsdf_sparse_ref.fuse(cams, dms, images, origin, voxel, dims, **kw)
    st = want["stats"]
    print("TSDF-SPARSE %s bricks=%d seed=%d allocated=%d vertices=%d faces=%d (device %d, %d)"
          % (label, st["bricks"], st["seed_bricks"], st["allocated_bricks"], len(want["xyz"]),
             len(want["faces"]), len(got["xyz"]), len(got["faces"])))
    assert np.array_equal(np.isnan(got["tsdf"]), np.isnan(want["tsdf"])), label
    assert np.array_equal(got["tsdf"], want["tsdf"], equal_nan=True), label
    _equal(got, want, ALL_KEYS, label)
    assert got["stats"] == st
    assert set(got) == set(want)
    return got


def _against_dense(hip, got, cams, depths, normals, images, box, cut, label, **kw):
    origin, voxel, dims = box
    dense = hip.fuse_tsdf(cams, depths, normals, images, origin, voxel, dims, cut=cut,
                          volume=True, **kw)
    cells = got["cells"]
    p = np.argsort(cells, kind="stable")
    for k in ("xyz", "normals", "rgb", "confidence"):
        assert np.array_equal(got[k][p], dense[k]), (label, k)
    # the dense active cells, from the dense volume
    idx, _ = tsdf_sparse_ref._active_cells(dense["tsdf"])
    assert np.array_equal(cells[p], (idx[2].astype(np.int64) * dims[1] + idx[1]) * dims[0]
                          + idx[0]), label
    rank = np.empty(len(p), np.int64)
    rank[p] = np.arange(len(p))
    a = rank[got["faces"].astype(np.int64)].reshape(-1, 3)
    b = dense["faces"].astype(np.int64)
    assert np.array_equal(a[np.lexsort(a.T[::-1])], b[np.lexsort(b.T[::-1])]), label
    # where allocated the volume is the dense one; elsewhere it is NaN / 0
    known = ~np.isnan(got["tsdf"])
    assert np.array_equal(got["tsdf"][known], dense["tsdf"][known]), label
    allocated = tsdf_sparse_ref._voxel_mask(got["brick_state"], got["tsdf"].shape)
    assert np.array_equal(got["weight"][allocated], dense["weight"][allocated]), label
    assert not known[~allocated].any() and not got["weight"][~allocated].any(), label
    return dense


@pytest.mark.parametrize("box", [SMALL, DEEP], ids=["37x29x23", "61x53x75"])
@pytest.mark.parametrize("n_views,channels,cut,min_weight", [
    (1, 3, True, 1), (3, 1, True, 1), (3, 3, False, 2), (5, 3, True, 2), (5, 1, False, 1)])
def test_sparse_fusion_matches_restatement_and_dense_entry(hip, oracle, box, n_views, channels,
                                                           cut, min_weight):
    cams, depths, normals, images = _inputs(n_views, 97, 63, channels)
    label = "%s-%dv-c%d-cut%d-mw%d" % (box[2], n_views, channels, cut, min_weight)
    got = _against_restatement(hip, oracle, cams, depths, normals, images, box, cut, label,
                               min_weight=min_weight)
    _against_dense(hip, got, cams, depths, normals, images, box, cut, label,
                   min_weight=min_weight)
    assert len(got["faces"]) > 100 and got["faces"].max() < len(got["xyz"])
    st = got["stats"]
    assert 0 < st["seed_bricks"] < st["allocated_bricks"] <= st["bricks"]
    if box is DEEP:
        assert 2 * st["allocated_bricks"] < st["bricks"]


@pytest.mark.parametrize("box", [SMALL, DEEP], ids=["37x29x23", "61x53x75"])
def test_a_view_of_another_size_and_an_explicit_truncation(hip, oracle, box):
    cams, depths, normals, images = _inputs(3, 97, 63, 3, last_size=(80, 71))
    assert depths[2].shape == (71, 80) != depths[0].shape
    got = _against_restatement(hip, oracle, cams, depths, normals, images, box, True,
                               "mixed-sizes", trunc=0.1)
    _against_dense(hip, got, cams, depths, normals, images, box, True, "mixed-sizes", trunc=0.1)
    assert len(got["faces"]) > 100


def test_two_cubed(hip, oracle):
    cams, depths, normals, images = _inputs(2, 97, 63, 3)
    box = ((-0.06, -0.06, 2.95), VOXEL, (2, 2, 2))
    got = _against_restatement(hip, oracle, cams, depths, normals, images, box, False, "2x2x2")
    _against_dense(hip, got, cams, depths, normals, images, box, False, "2x2x2")
    assert len(got["xyz"]) == 1 and len(got["faces"]) == 0
    assert got["brick_state"].shape == (1, 1, 1) and got["brick_state"][0, 0, 0] == 2


def test_box_in_free_space(hip, oracle):
    # no voxel within the band of any view: no seed, nothing allocated, no error
    cams, depths, normals, images = _inputs(2, 97, 63, 3)
    box = ((-0.3, -0.2, 1.0), 0.03, (9, 8, 7))
    got = _against_restatement(hip, oracle, cams, depths, normals, images, box, True,
                               "free-space")
    assert got["xyz"].shape == (0, 3) and got["faces"].shape == (0, 3)
    assert got["cells"].shape == (0,)
    assert got["stats"] == {"bricks": 4, "seed_bricks": 0, "allocated_bricks": 0,
                            "state_bytes": 0}
    assert np.isnan(got["tsdf"]).all() and not got["weight"].any()


def test_box_half_outside_every_frustum(hip, oracle):
    cams, depths, normals, images = _inputs(5, 97, 63, 3)
    box = ((-1.0, -0.2, 2.8), VOXEL, (37, 29, 23))
    got = _against_restatement(hip, oracle, cams, depths, normals, images, box, True,
                               "half-outside")
    _against_dense(hip, got, cams, depths, normals, images, box, True, "half-outside")
    assert np.isnan(got["tsdf"][:, -3:, :]).all()
    assert len(got["faces"]) > 100


def test_box_around_a_camera_centre(hip, oracle):
    cams, depths, normals, images = _inputs(5, 97, 63, 1)
    box = ((-0.6, -0.5, -0.62), 0.15, (8, 7, 41))
    centre = np.asarray(cams[1].center)
    assert np.all(centre > box[0]) \
        and np.all(centre < np.asarray(box[0]) + box[1] * np.array(box[2]))
    got = _against_restatement(hip, oracle, cams, depths, normals, images, box, True,
                               "camera-inside")
    _against_dense(hip, got, cams, depths, normals, images, box, True, "camera-inside")
    assert np.all(got["brick_state"][0] == 0)          # z < 0: behind every camera
    assert len(got["faces"]) > 0


# ------------------------------------------------- beyond the dense entry's limits
def test_a_side_of_4096(hip, oracle):
    """4096 x 16 x 12 voxels: a thin bar across the sphere's front, which
    crosses its long axis obliquely twice."""
    from smvs_amd._capi import SmvsError
    cams, depths, normals, images = _inputs(2, 97, 63, 3)
    box = ((-1.2, -0.005, 3.1), 0.0006, (4096, 16, 12))
    with pytest.raises(SmvsError):
        hip.fuse_tsdf(cams, depths, normals, images, *box, cut=True)
    got = _against_restatement(hip, oracle, cams, depths, normals, images, box, True, "4096")
    assert len(got["faces"]) > 100
    i = got["cells"] % 4096
    assert i.min() < 2048 < i.max()
    assert got["stats"]["allocated_bricks"] < got["stats"]["bricks"]


# the sphere's front (z = 3 on the axis, farther off it) from k = 250 up to the
# box's top: cells on both sides of 2^32 = 256 * 4096 * 4096
HUGE = ((-4.1, -4.1, 2.499), 0.002, (4096, 4096, 264))
HUGE_WINDOW = ((1920, 1952, 232), (2176, 2144, 264))


def test_more_than_2_to_the_32_voxels(hip):
    """4096 x 4096 x 264 voxels and one narrow 32 x 24 view: no brick outside
    the window its frustum meets is allocated; inside it the mesh, the cells
    (above 2^32 too) and the stats are the restatement's from field_window."""
    from smvs_amd import synth
    origin, voxel, dims = HUGE
    assert dims[0] * dims[1] * dims[2] > 1 << 32
    cam = synth.Camera(np.eye(3), np.zeros(3), 8.0, 32, 24)
    depths, normals = synth.depth_and_normal_maps(synth.SphereScene(), [cam])
    rng = np.random.default_rng(3)
    images = [rng.integers(0, 256, (24, 32, 3)).astype(np.uint8)]
    depths[0][5, 7] = 0.0
    got = hip.fuse_tsdf([cam], depths, normals, images, origin, voxel, dims, cut=True,
                        sparse=True, brick_state=True)
    want = tsdf_sparse_ref.fuse([cam], depths, images, origin, voxel, dims, window=HUGE_WINDOW)
    lo, hi = HUGE_WINDOW
    outside = got["brick_state"].copy()
    outside[lo[2] // 4:hi[2] // 4, lo[1] // 8:hi[1] // 8, lo[0] // 8:hi[0] // 8] = 0
    assert not outside.any()
    print("TSDF-SPARSE huge", want["stats"], "vertices", len(want["xyz"]), "faces",
          len(want["faces"]), "max cell", int(want["cells"].max()))
    _equal(got, want, ("brick_state",) + MESH_KEYS + ("cells",), "huge")
    assert got["stats"] == want["stats"]
    assert len(got["faces"]) > 100
    assert got["cells"].min() < 1 << 32 < got["cells"].max()


# ------------------------------------------------------------------- the budget
def test_budget(hip, oracle):
    from smvs_amd._capi import SmvsError
    cams, depths, normals, images = _inputs(3, 97, 63, 3)
    origin, voxel, dims = DEEP
    full = hip.fuse_tsdf(cams, depths, normals, images, origin, voxel, dims, sparse=True)
    need = full["stats"]["allocated_bricks"]
    assert need > 1
    with pytest.raises(SmvsError) as e:
        hip.fuse_tsdf(cams, depths, normals, images, origin, voxel, dims, sparse=True,
                      max_bricks=need - 1)
    assert e.value.status == -4 and str(need) in str(e.value)
    assert e.value.stats == full["stats"]
    exact = hip.fuse_tsdf(cams, depths, normals, images, origin, voxel, dims, sparse=True,
                          max_bricks=need)
    _equal(exact, full, MESH_KEYS + ("cells",), "budget")


def test_budget_leaves_no_handle(hip):
    """the C entry itself: SMVS_ERR_NOMEM, the stats filled, the handle NULL"""
    import ctypes as C
    from smvs_amd import _capi
    from smvs_amd.device import _tsdf_views
    cams, depths, normals, images = _inputs(2, 97, 63, 3)
    lib = _capi.load()
    arr, _keep = _tsdf_views(cams, depths, normals, images)
    opt = _capi.TsdfOptions()
    opt.cut_surfaces = 1
    opt.voxel_size = VOXEL
    for k in range(3):
        opt.origin[k] = SMALL[0][k]
        opt.dims[k] = SMALL[2][k]
    sopt = _capi.TsdfSparseOptions()
    sopt.max_bricks = 1
    stats = _capi.TsdfSparseStats()
    handle = C.c_void_p(1)
    nv, nf = C.c_int64(-7), C.c_int64(-7)
    rc = lib.smvs_tsdf_fuse_sparse(0, arr, 2, C.byref(opt), C.byref(sopt), None, None, None,
                                   C.byref(stats), C.byref(handle), C.byref(nv), C.byref(nf))
    assert rc == -4 and handle.value is None
    assert stats.bricks == 5 * 4 * 6 and 1 < stats.seed_bricks < stats.allocated_bricks
    assert stats.state_bytes == stats.allocated_bricks * 256 * 28
    # a dense handle has no cells
    dense = C.c_void_p()
    assert lib.smvs_tsdf_fuse(0, arr, 2, C.byref(opt), None, None, C.byref(dense), C.byref(nv),
                              C.byref(nf)) == 0
    try:
        cells = (C.c_int64 * max(nv.value, 1))()
        assert lib.smvs_tsdf_vertex_cells(dense, cells) == -1
    finally:
        lib.smvs_points_release(dense)


# -------------------------------------------------------------- the scene entry
def test_scene_fused_sparse(hip, tmp_path):
    """host.generate_fused(scene, sparse=True) writes what the C ABI gives for
    the saved embeddings and the same box."""
    from smvs_amd import synth, host, mve_scene
    inputs = synth.pipeline_inputs("sphere", 192, 128, 2, flen=1.2)
    d = str(tmp_path)
    mve_scene.write_scene(d, inputs)
    done, _, _ = host.reconstruct_scene(d, view_ids=[0, 1, 2], num_neighbors=2,
                                        min_neighbors=1, output_scale=2, input_scale=0)
    assert sorted(done) == [0, 1, 2]
    cams = inputs["cams"][:3]
    vdirs = [os.path.join(d, "views", "view_%04d.mve" % i) for i in range(3)]
    depths = [mve_scene.load_mvei(os.path.join(v, "smvs-B0.mvei")) for v in vdirs]
    normals = [mve_scene.load_mvei(os.path.join(v, "smvs-B0N.mvei")) for v in vdirs]
    images = [mve_scene.load_mvei(os.path.join(v, "undistorted.mvei")) for v in vdirs]
    lo, hi = np.float32((-1.0, -0.8, 2.8)), np.float32((1.0, 0.8, 4.3))
    voxel = np.float32(0.05)
    path, nv, nf = host.generate_fused(d, voxel_size=voxel, aabb=(lo, hi), input_scale=0,
                                       sparse=True)
    assert os.path.basename(path) == "smvs-fused-B0.ply" and os.path.dirname(path) == d
    dims = [max(2, int(np.ceil((hi[a] - lo[a]) / voxel))) for a in range(3)]
    want = hip.fuse_tsdf(cams, depths, normals, images, lo, voxel, dims, cut=True, sparse=True)
    lines, props, faces = mesh_ref.read_ply_mesh(path)
    assert "element vertex %d" % nv in lines and "element face %d" % nf in lines
    got = {"xyz": np.stack([props["x"], props["y"], props["z"]], 1),
           "normals": np.stack([props["nx"], props["ny"], props["nz"]], 1),
           "rgb": np.stack([props["red"], props["green"], props["blue"]], 1),
           "confidence": props["confidence"], "faces": faces.astype(np.uint32)}
    assert nf > 100
    for k in MESH_KEYS:
        assert np.array_equal(got[k], want[k]), k
    # the budget reaches the scene entry
    with pytest.raises(Exception):
        host.generate_fused(d, voxel_size=voxel, aabb=(lo, hi), input_scale=0, sparse=True,
                            max_bricks=1)
