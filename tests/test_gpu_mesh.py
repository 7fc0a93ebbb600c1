"""smvs_mesh_generate (smvsrecon --mesh on the device) against the serial CPU
restatement tests/mesh_reference.cc, run on the oracle's cut maps: positions,
colours, confidences, faces and the vertex order identical; the vertex normals
within 1e-6 (the device's acosf and the host's need not agree to the bit)."""
import ctypes as C
import os

import numpy as np
import pytest

import mesh_ref  # tests/mesh_ref.py
import points_ref  # tests/points_ref.py

pytestmark = pytest.mark.gpu

EXACT = ("xyz", "rgb", "confidence", "faces")
NORMAL_TOL = 1e-6


@pytest.fixture(scope="module")
def hip():
    import smvs_amd
    if smvs_amd.device_count() < 1:
        pytest.fail("no HIP device")
    return smvs_amd


def _inputs(n_views, w, h, channels, seed=5, kind="sphere"):
    from smvs_amd import synth
    inputs = synth.pipeline_inputs(kind, w, h, max(n_views - 1, 1), flen=1.2)
    cams = inputs["cams"][:n_views]
    depths, normals = synth.depth_and_normal_maps(inputs["scene"], cams)
    rng = np.random.default_rng(seed)
    for i in range(n_views):
        depths[i] *= (1.0 + 0.002 * rng.standard_normal(depths[i].shape)).astype(np.float32)
        depths[i][rng.random(depths[i].shape) < 0.01] = 0.0          # holes
    depths[0][h // 5:h // 5 + 9, w // 4:w // 4 + 13] *= np.float32(0.8)   # a step
    images = [rng.integers(0, 256, (h, w) if channels == 1 else (h, w, channels))
              .astype(np.uint8) for _ in range(n_views)]
    return inputs["scene"], cams, depths, normals, images


def _cut_maps(oracle, cams, depths, normals, cut):
    if cut and len(cams) > 1:
        return oracle.cut_depth_maps(cams, depths, normals)
    dms, wn = [], []
    for c, d, n in zip(cams, depths, normals):
        a, b = oracle.cut_depth_maps([c], [d], [n])
        dms.append(a[0])
        wn.append(b[0])
    return dms, wn


def _reference(oracle, cams, depths, normals, images, cut, aabb=None):
    dms, wn = _cut_maps(oracle, cams, depths, normals, cut)
    return mesh_ref.mesh(cams, dms, wn, images, aabb=aabb), dms


def _assert_same(got, want, label):
    assert len(got["xyz"]) == len(want["xyz"]) > 0
    assert len(got["faces"]) == len(want["faces"]) > 0
    for k in EXACT:
        assert np.array_equal(got[k], want[k]), k
    assert "value" not in got
    d = np.abs(got["normals"].astype(np.float64) - want["normals"])
    differing = int((d.max(axis=1) > 0).sum())
    print("MESH_NORMALS %s vertices=%d faces=%d max_abs_diff=%.3g differing=%d"
          % (label, len(got["xyz"]), len(got["faces"]), d.max(), differing))
    assert d.max() <= NORMAL_TOL
    # zero exactly where the restatement has no normal (M5)
    assert np.array_equal(np.all(got["normals"] == 0, axis=1),
                          np.all(want["normals"] == 0, axis=1))


@pytest.mark.parametrize("n_views,w,h,channels,cut", [
    (1, 96, 64, 3, True), (2, 97, 63, 1, True), (2, 97, 63, 3, False),
    (9, 161, 121, 3, True), (9, 161, 121, 1, False)])
def test_mesh_matches_restatement(hip, oracle, n_views, w, h, channels, cut):
    _, cams, depths, normals, images = _inputs(n_views, w, h, channels)
    got = hip.generate_mesh(cams, depths, normals, images, cut=cut, cut_maps=True)
    want, dms = _reference(oracle, cams, depths, normals, images, cut)
    _assert_same(got, want, "%dx%dx%d-c%d-cut%d" % (n_views, w, h, channels, cut))
    for a, b in zip(got["cut_depth"], dms):
        assert np.array_equal(a, b)
    assert got["faces"].max() < len(got["xyz"])


def _view_of_vertices(cams, dms, images):
    counts = [len(points_ref.view(c, d, np.zeros(d.shape + (3,), np.float32), i)["xyz"])
              for c, d, i in zip(cams, dms, images)]
    return np.repeat(np.arange(len(counts)), counts)


@pytest.mark.parametrize("cut,channels", [(True, 3), (False, 1)])
def test_mesh_aabb_cuts_faces_in_every_view(hip, oracle, cut, channels):
    _, cams, depths, normals, images = _inputs(3, 128, 96, channels, seed=8)
    aabb = ((-0.6, -0.5, 0.0), (0.7, 0.6, 4.5))
    got = hip.generate_mesh(cams, depths, normals, images, cut=cut, aabb=aabb)
    want, dms = _reference(oracle, cams, depths, normals, images, cut, aabb=aabb)
    _assert_same(got, want, "aabb-cut%d-c%d" % (cut, channels))
    # the box removes faces and keeps faces in every view, and some vertices
    # lose all their faces (kept, normal 0)
    full = hip.generate_mesh(cams, depths, normals, images, cut=cut)
    view = _view_of_vertices(cams, dms, images)
    lo, hi = np.float32(aabb[0]), np.float32(aabb[1])
    inside = ~((full["xyz"] < lo) | (full["xyz"] > hi)).any(axis=1)
    fkeep = inside[full["faces"]].all(axis=1)
    fview = view[full["faces"][:, 0]]
    for v in range(3):
        assert 0 < fkeep[fview == v].sum() < (fview == v).sum(), v
    assert len(got["xyz"]) == inside.sum() < len(full["xyz"])
    assert len(got["faces"]) == fkeep.sum()
    assert np.any(np.all(got["normals"] == 0, axis=1))


def test_mesh_box_around_everything_changes_nothing(hip):
    """The shared AABB clip with a box that holds every vertex (the unclipped
    min / max, one float step outward): bit for bit the unclipped mesh."""
    _, cams, depths, normals, images = _inputs(3, 128, 96, 3, seed=8)
    full = hip.generate_mesh(cams, depths, normals, images, cut=True)
    assert len(full["xyz"]) > 4096          # more than one scan tile
    lo = np.nextafter(full["xyz"].min(axis=0), np.float32(-np.inf))
    hi = np.nextafter(full["xyz"].max(axis=0), np.float32(np.inf))
    got = hip.generate_mesh(cams, depths, normals, images, cut=True, aabb=(lo, hi))
    assert sorted(got) == sorted(full)
    for k in ("xyz", "normals", "rgb", "confidence", "faces"):
        assert got[k].dtype == full[k].dtype and got[k].shape == full[k].shape, k
        assert got[k].tobytes() == full[k].tobytes(), k


def test_mesh_full_size_nine_views(hip, oracle):
    _, cams, depths, normals, images = _inputs(9, 1920, 1080, 3, seed=11)
    got = hip.generate_mesh(cams, depths, normals, images, cut=True)
    want, _ = _reference(oracle, cams, depths, normals, images, True)
    _assert_same(got, want, "9x1920x1080")


def test_mesh_normals_agree_with_the_normal_maps(hip):
    # independent of the restatement: on the synthetic sphere and plane, the
    # mesh normals of interior vertices (confidence 1) and the looked-up
    # normal-map normals of the point cloud (P12) agree up to one global sign
    from smvs_amd import synth
    inputs = synth.pipeline_inputs("sphere", 320, 240, 4, flen=1.2)
    cams = inputs["cams"]
    depths, normals = synth.depth_and_normal_maps(inputs["scene"], cams)
    images = [np.zeros((240, 320), np.uint8) for _ in cams]
    m = hip.generate_mesh(cams, depths, normals, images, cut=False)
    p = hip.generate_points(cams, depths, normals, images, cut=False)
    assert np.array_equal(m["xyz"], p["xyz"])
    interior = m["confidence"] == 1.0
    assert interior.sum() > 0.5 * len(m["xyz"])
    a = m["normals"][interior].astype(np.float64)
    b = p["normals"][interior].astype(np.float64)
    cos = (a * b).sum(axis=1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
    sign = np.sign(np.median(cos))
    frac = float(np.mean(sign * cos > 0.99))
    print("MESH_NORMAL_SIGN sign=%+d fraction=%.5f interior=%d" % (sign, frac, len(cos)))
    assert sign == 1.0       # both face the cameras
    assert frac >= 0.99


def test_point_path_unchanged(hip, oracle):
    _, cams, depths, normals, images = _inputs(3, 128, 96, 3, seed=8)
    got = hip.generate_points(cams, depths, normals, images, cut=True, faces=True)
    dms, wn = _cut_maps(oracle, cams, depths, normals, True)
    want = points_ref.points(cams, dms, wn, images)
    for k in ("xyz", "normals", "rgb", "confidence", "value", "faces"):
        assert np.array_equal(got[k], want[k]), k
    m = hip.generate_mesh(cams, depths, normals, images, cut=True)
    for k in ("xyz", "rgb", "confidence", "faces"):
        assert np.array_equal(m[k], got[k]), k
    again = hip.generate_points(cams, depths, normals, images, cut=True, faces=True)
    for k in got:
        assert np.array_equal(again[k], got[k]), k


def test_mesh_rejects_bad_arguments(hip):
    from smvs_amd import _capi
    from smvs_amd._capi import SmvsError
    from smvs_amd.device import _point_views
    _, cams, depths, normals, images = _inputs(2, 64, 48, 3)
    with pytest.raises(SmvsError):
        hip.generate_mesh([], [], [], [])
    with pytest.raises(SmvsError):
        hip.generate_mesh(cams, depths, normals, images, dd_factor=-1.0)
    with pytest.raises(ValueError):
        hip.generate_mesh(cams, depths, normals, [images[0][:10]] * 2)
    # a mesh handle has no values
    lib = _capi.load()
    arr, _, _keep = _point_views(cams, depths, normals, images, False)
    handle, nv, nf = C.c_void_p(), C.c_int64(), C.c_int64()
    _capi.check(lib.smvs_mesh_generate(0, arr, 2, None, C.byref(handle), C.byref(nv),
                                       C.byref(nf)))
    try:
        got_v, got_f = C.c_int64(), C.c_int64()
        _capi.check(lib.smvs_points_info(handle, C.byref(got_v), C.byref(got_f)))
        assert (got_v.value, got_f.value) == (nv.value, nf.value) and nf.value > 0
        value = np.zeros(nv.value, np.float32)
        assert lib.smvs_points_download(handle, None, None, None, None,
                                        value.ctypes.data_as(C.POINTER(C.c_float)),
                                        None) != 0
        faces = np.zeros((nf.value, 3), np.uint32)
        _capi.check(lib.smvs_points_download(handle, None, None, None, None, None,
                                             faces.ctypes.data_as(C.POINTER(C.c_uint32))))
    finally:
        lib.smvs_points_release(handle)
    # NULL options = the reference's defaults (cut, no AABB, dd_factor 5)
    assert np.array_equal(faces, hip.generate_mesh(cams, depths, normals, images)["faces"])


def test_scene_mesh_end_to_end(hip, oracle, tmp_path):
    """mve_scene.write_scene -> host.reconstruct_scene (3 views) ->
    host.generate_mesh: smvsrecon's smvs-m-B0.ply, its contents equal to the
    restatement on the saved embeddings; the point-cloud entry still refuses
    --mesh and the mesh entry --simplify."""
    from smvs_amd import synth, host, mve_scene
    from smvs_amd._capi import SmvsError
    inputs = synth.pipeline_inputs("sphere", 192, 128, 2, flen=1.2)
    d = str(tmp_path)
    mve_scene.write_scene(d, inputs)
    done, _, _ = host.reconstruct_scene(d, view_ids=[0, 1, 2], num_neighbors=2,
                                        min_neighbors=1, output_scale=2, input_scale=0)
    assert sorted(done) == [0, 1, 2]
    path, nv, nf = host.generate_mesh(d, input_scale=0)
    assert os.path.basename(path) == "smvs-m-B0.ply" and os.path.dirname(path) == d
    lines, props, faces = mesh_ref.read_ply_mesh(path)
    assert "element vertex %d" % nv in lines and "element face %d" % nf in lines
    assert "property float value" not in lines
    cams = inputs["cams"][:3]
    vdirs = [os.path.join(d, "views", "view_%04d.mve" % i) for i in range(3)]
    depths = [mve_scene.load_mvei(os.path.join(v, "smvs-B0.mvei")) for v in vdirs]
    normals = [mve_scene.load_mvei(os.path.join(v, "smvs-B0N.mvei")) for v in vdirs]
    images = [mve_scene.load_mvei(os.path.join(v, "undistorted.mvei")) for v in vdirs]
    want, _ = _reference(oracle, cams, depths, normals, images, True)
    got = {"xyz": np.stack([props["x"], props["y"], props["z"]], 1),
           "normals": np.stack([props["nx"], props["ny"], props["nz"]], 1),
           "rgb": np.stack([props["red"], props["green"], props["blue"]], 1),
           "confidence": props["confidence"], "faces": faces.astype(np.uint32)}
    _assert_same(got, want, "scene")
    cut_d, _ = hip.cut_depth_maps(cams, depths, normals)
    for v, c in zip(vdirs, cut_d):
        assert np.array_equal(mve_scene.load_mvei(os.path.join(v, "smvs-cut.mvei")), c)
    # the point cloud next to it is untouched by the mesh
    ppath, n = host.generate_point_cloud(d, input_scale=0)
    assert os.path.basename(ppath) == "smvs-B0.ply" and n == nv
    with pytest.raises(SmvsError):
        host.generate_point_cloud(d, input_scale=0, mesh=True)
    with pytest.raises(SmvsError):
        host.generate_mesh(d, input_scale=0, simplify=True)
