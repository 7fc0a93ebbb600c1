"""The mesh clean on the MI355X (smvs_mesh_clean)
against the numpy restatement of its definition (tests/mesh_clean_ref.py) on
the cases of tests/mesh_clean_cases.py, on the suite's own fused mesh, and
through the host's scene entry.  Everything the definition fixes is a fact of
the input, so every comparison is for equality."""
import ctypes as C
import os

import numpy as np
import pytest

import mesh_clean_cases as cases  # tests/mesh_clean_cases.py
import mesh_clean_ref as ref  # tests/mesh_clean_ref.py
import test_gpu_tsdf as tsdf_tests  # the suite's fusion inputs
from test_mesh_clean_cpu import REFUSED, call_clean

pytestmark = pytest.mark.gpu

MESH_KEYS = ("xyz", "normals", "rgb", "confidence", "faces")


@pytest.fixture(scope="module")
def hip():
    import smvs_amd
    if smvs_amd.device_count() < 1:
        pytest.fail("no HIP device")
    return smvs_amd


def without_cells(mesh):
    return {k: v for k, v in mesh.items() if k != "cells"}


@pytest.mark.parametrize("with_cells", [False, True], ids=["plain", "cells"])
@pytest.mark.parametrize("name", cases.case_names())
def test_case_matches_restatement(hip, name, with_cells):
    mesh, opts, want = cases.case(name)
    got = hip.clean_mesh(mesh if with_cells else without_cells(mesh), labels=True, **opts)
    # (with cells the download goes through smvs_tsdf_vertex_cells on the result)
    assert ("cells" in got) == with_cells
    ref.assert_same(got, want, cells=with_cells)
    assert set(got) == set(want) - (set() if with_cells else {"cells"})
    # without labels: the same mesh
    plain = hip.clean_mesh(mesh if with_cells else without_cells(mesh), **opts)
    assert set(plain) == set(got) - {"component", "component_size", "new_id"}
    for k in MESH_KEYS:
        assert np.array_equal(plain[k].view(np.uint8), got[k].view(np.uint8)), k
    assert plain["stats"]["n_components"] == want["stats"]["n_components"]


def test_handles(hip):
    """the result is sparse exactly when cells was given; smvs_mesh_clean_handle
    cleans what a handle holds and refuses a handle without faces"""
    from smvs_amd import _capi
    lib = _capi.load()
    mesh, opts, want = cases.case("groups-257-dense")
    fp, u8p, u32p, i64p = (C.POINTER(t) for t in (C.c_float, C.c_uint8, C.c_uint32, C.c_int64))
    opt = _capi.MeshCleanOptions(opts["threshold"], 0.0, opts["component_size"], 0)
    n, m = mesh["confidence"].size, mesh["faces"].shape[0]

    def clean(cells):
        h, nv, nf = C.c_void_p(), C.c_int64(), C.c_int64()
        assert lib.smvs_mesh_clean(
            0, C.c_int64(n), C.c_int64(m), mesh["xyz"].ctypes.data_as(fp),
            mesh["normals"].ctypes.data_as(fp), mesh["rgb"].ctypes.data_as(u8p),
            mesh["confidence"].ctypes.data_as(fp),
            cells.ctypes.data_as(i64p) if cells is not None else None,
            mesh["faces"].ctypes.data_as(u32p), C.byref(opt), None, None, None, None,
            C.byref(h), C.byref(nv), C.byref(nf)) == 0
        assert (nv.value, nf.value) == (want["confidence"].size, want["faces"].shape[0])
        return h, nv.value

    plain, k = clean(None)
    sparse, _ = clean(mesh["cells"])
    out = np.zeros(k, np.int64)
    try:
        assert lib.smvs_tsdf_vertex_cells(plain, out.ctypes.data_as(i64p)) == -1
        assert lib.smvs_tsdf_vertex_cells(sparse, out.ctypes.data_as(i64p)) == 0
        assert np.array_equal(out, want["cells"])
        # cleaning the cleaned handle with everything off gives it back
        off = _capi.MeshCleanOptions(0.0, 0.0, 1, 0)
        stats = _capi.MeshCleanStats()
        again, nv, nf = C.c_void_p(), C.c_int64(), C.c_int64()
        assert lib.smvs_mesh_clean_handle(0, sparse, C.byref(off), None, None, None,
                                          C.byref(stats), C.byref(again), C.byref(nv),
                                          C.byref(nf)) == 0
        try:
            assert (nv.value, nf.value) == (k, want["faces"].shape[0])
            faces = np.zeros((nf.value, 3), np.uint32)
            conf = np.zeros(k, np.float32)
            assert lib.smvs_points_download(again, None, None, None, conf.ctypes.data_as(fp),
                                            None, faces.ctypes.data_as(u32p)) == 0
            assert np.array_equal(faces, want["faces"])
            assert np.array_equal(conf, want["confidence"])
            assert lib.smvs_tsdf_vertex_cells(again, out.ctypes.data_as(i64p)) == 0
            assert np.array_equal(out, want["cells"])
            assert stats.n_cut == 0 and stats.cut_value == -np.inf
        finally:
            lib.smvs_points_release(again)
    finally:
        lib.smvs_points_release(plain)
        lib.smvs_points_release(sparse)
    # a point cloud's handle that kept no faces
    from smvs_amd import device
    cams, depths, normals, images = tsdf_tests._inputs(2, 97, 63, 3)
    arr, _cuts, _keep = device._point_views(cams, depths, normals, images, False)
    popt = device.PointsOptions()
    popt.cut_surfaces, popt.dd_factor, popt.want_faces = 1, 5.0, 0
    pts, nv = C.c_void_p(), C.c_int64()
    assert lib.smvs_points_generate(0, arr, 2, C.byref(popt), C.byref(pts), C.byref(nv)) == 0
    try:
        h = C.c_void_p()
        assert nv.value > 0
        assert lib.smvs_mesh_clean_handle(0, pts, C.byref(off), None, None, None, None,
                                          C.byref(h), None, None) == -1
        assert b"no faces" in lib.smvs_last_error() and not h.value
    finally:
        lib.smvs_points_release(pts)


@pytest.mark.parametrize("how", REFUSED, ids=lambda h: "-".join("%s=%s" % kv for kv in h.items()))
def test_refused(hip, how):
    from smvs_amd import _capi
    assert call_clean(_capi.load(), _capi, cases.small_mesh(), **how) == -1


def test_refused_face_id(hip):
    mesh = cases.small_mesh()
    for bad in (10, 11):   # 10 == n
        faces = mesh["faces"].copy()
        faces[1, 0] = bad
        with pytest.raises(hip._capi.SmvsError) as e:
            hip.clean_mesh(dict(mesh, faces=faces))
        assert e.value.status == -1 and "vertex id" in str(e.value)
    with pytest.raises(hip._capi.SmvsError) as e:
        hip.clean_mesh(mesh, threshold=0.1, percentile=10.0)
    assert e.value.status == -1


@pytest.fixture(scope="module")
def fused(hip):
    """the suite's fusion (tests/test_gpu_tsdf.py: 5 views of 97 x 63, the box
    DIMS), dense and sparse"""
    cams, depths, normals, images = tsdf_tests._inputs(5, 97, 63, 3)
    box = (tsdf_tests.SURFACE_BOX, tsdf_tests.VOXEL, tsdf_tests.DIMS)
    return {sparse: hip.fuse_tsdf(cams, depths, normals, images, *box, cut=True, sparse=sparse)
            for sparse in (False, True)}


CLEAN = dict(percentile=10, component_size=50)


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_fused_mesh(hip, fused, sparse):
    mesh = {k: v for k, v in fused[sparse].items() if k in MESH_KEYS + ("cells",)}
    assert len(mesh["faces"]) > 100 and ("cells" in mesh) == sparse
    want = ref.clean(mesh, **CLEAN)
    got = hip.clean_mesh(mesh, labels=True, **CLEAN)
    print("CLEAN fused %s: %d -> %d vertices, %d -> %d faces, %s"
          % ("sparse" if sparse else "dense", len(mesh["xyz"]), len(got["xyz"]),
             len(mesh["faces"]), len(got["faces"]), got["stats"]))
    ref.assert_same(got, want, cells=sparse)
    # the case is not vacuous: the cut and the components both remove something
    assert got["stats"]["n_cut"] > 0 and got["stats"]["n_small_vertices"] > 0
    assert len(got["faces"]) > 100
    assert got["faces"].max() < len(got["xyz"])
    used = np.zeros(len(got["xyz"]), bool)
    used[got["faces"].astype(np.int64).ravel()] = True
    assert used.all()
    # cleaning the result again with the cut off returns it unchanged
    again = hip.clean_mesh({k: got[k] for k in mesh}, **CLEAN | dict(percentile=0))
    for k in mesh:
        assert np.array_equal(again[k].view(np.uint8), got[k].view(np.uint8)), k


def test_fused_dense_and_sparse_agree(hip, fused):
    """the same set of vertices, sorted by cell"""
    dense = hip.clean_mesh({k: fused[False][k] for k in MESH_KEYS}, labels=True, **CLEAN)
    sparse = hip.clean_mesh({k: fused[True][k] for k in MESH_KEYS + ("cells",)}, **CLEAN)
    # dense ids run in cell order: the cell of a dense vertex is the rank's cell
    order = np.argsort(fused[True]["cells"], kind="stable")
    assert np.array_equal(fused[True]["xyz"][order], fused[False]["xyz"])
    dense_cells = fused[True]["cells"][order][dense["new_id"] >= 0]
    by_cell = np.argsort(sparse["cells"], kind="stable")
    assert np.array_equal(sparse["cells"][by_cell], dense_cells)
    for k in ("xyz", "normals", "rgb", "confidence"):
        assert np.array_equal(sparse[k][by_cell].view(np.uint8), dense[k].view(np.uint8)), k
    assert len(sparse["faces"]) == len(dense["faces"])
    assert sparse["stats"] == dense["stats"]


def test_scene_fused_clean(hip, tmp_path):
    """host.generate_fused(clean=...) writes save_ply_mesh of
    clean_mesh(fuse_tsdf(...)) as smvs-clean-B0.ply and returns its counts;
    with clean=None the fused file is what it was."""
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
    dims = [max(2, int(np.ceil((hi[a] - lo[a]) / voxel))) for a in range(3)]

    def file_of(mesh, name):
        path = os.path.join(d, name)
        host.save_ply_mesh(path, *(mesh[k] for k in MESH_KEYS))
        with open(path, "rb") as f:
            return f.read()

    for kw in (dict(), dict(sparse=True), dict(sparse=True, cull=True)):
        fkw = dict(sparse=True) if kw else {}
        want_fused = hip.fuse_tsdf(cams, depths, normals, images, lo, voxel, dims, cut=True, **fkw)
        want = hip.clean_mesh(want_fused, **CLEAN)
        fused_path = os.path.join(d, "smvs-fused-B0.ply")
        if os.path.exists(fused_path):
            os.remove(fused_path)
        path, nv, nf, stats = host.generate_fused(d, voxel_size=voxel, aabb=(lo, hi),
                                                  input_scale=0, clean=CLEAN, **kw)
        assert os.path.basename(path) == "smvs-clean-B0.ply" and os.path.dirname(path) == d
        assert not os.path.exists(fused_path)
        assert (nv, nf) == (len(want["xyz"]), len(want["faces"])) and nf > 100
        assert nv < len(want_fused["xyz"])
        assert np.float32(stats.pop("cut_value")) == np.float32(want["stats"].pop("cut_value"))
        assert stats == want["stats"]
        with open(path, "rb") as f:
            assert f.read() == file_of(want, "want-clean.ply")
        # clean=None: the fused file, byte for byte the fusion's
        path, nv, nf = host.generate_fused(d, voxel_size=voxel, aabb=(lo, hi), input_scale=0,
                                           **kw)
        assert path == fused_path and (nv, nf) == (len(want_fused["xyz"]),
                                                   len(want_fused["faces"]))
        with open(path, "rb") as f:
            assert f.read() == file_of(want_fused, "want-fused.ply")
