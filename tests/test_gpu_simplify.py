"""smvsrecon --simplify on the device against the
serial CPU restatement tests/simplify_reference.cc: the raw greedy
triangulation insertion by insertion, the exported point cloud and mesh, and
the scene entry end to end.  An insertion order that differs is a failure:
everything but the mesh's recalc_normals is compared with array_equal."""
import os

import numpy as np
import pytest

import mesh_ref  # tests/mesh_ref.py
import points_ref  # tests/points_ref.py
import simplify_ref  # tests/simplify_ref.py

pytestmark = pytest.mark.gpu

# recalc_normals: the project's bound for acosf on the device
NORMAL_TOL = 1e-6


@pytest.fixture(scope="module")
def hip():
    import smvs_amd
    if smvs_amd.device_count() < 1:
        pytest.fail("no HIP device")
    return smvs_amd


def _map(w, h, holes=True, seed=3):
    """A sphere in front of a plane, noise, and (holes) zeros: single pixels
    and a block."""
    from smvs_amd import synth
    inputs = synth.pipeline_inputs("sphere", w, h, 1, flen=1.2)
    depths, _ = synth.depth_and_normal_maps(inputs["scene"], inputs["cams"][:1])
    rng = np.random.default_rng(seed)
    d = depths[0] * (1.0 + 0.002 * rng.standard_normal((h, w))).astype(np.float32)
    if holes:
        d[rng.random((h, w)) < 0.01] = 0.0
        d[h // 3:h // 3 + 7, w // 2:w // 2 + 11] = 0.0
    return np.ascontiguousarray(d, np.float32)


def _assert_same_triangulation(got, want, label):
    print("SIMPLIFY_TRI %s iterations=%d/%d vertices=%d triangles=%d"
          % (label, got["iterations"], want["iterations"], len(got["vertices"]),
             len(got["triangles"])))
    assert got["iterations"] == want["iterations"]
    n = min(len(got["vertices"]), len(want["vertices"]))
    differ = np.nonzero((got["vertices"][:n] != want["vertices"][:n]).any(axis=1))[0]
    assert len(differ) == 0, "first differing insertion: vertex %d" % differ[0]
    assert len(got["vertices"]) == len(want["vertices"])
    assert np.array_equal(got["triangles"], want["triangles"])
    assert np.array_equal(got["num_zero_depths"], want["num_zero_depths"])


@pytest.mark.parametrize("w,h,holes", [(97, 63, False), (97, 63, True), (161, 121, True),
                                       (480, 270, True)])
def test_triangulation_matches_restatement(hip, w, h, holes):
    dm = _map(w, h, holes)
    got = hip.simplify_triangulate(dm)
    want = simplify_ref.triangulate(dm)
    _assert_same_triangulation(got, want, "%dx%d-holes%d" % (w, h, holes))
    if (w, h) == (480, 270):
        assert want["iterations"] == 3240   # noise: the error bound is never reached


def test_triangulation_with_explicit_bounds(hip):
    """max_vertices and max_error on both sides of where the loop would stop by
    itself (a roof of four planes stops on its error bound before the budget)."""
    dm = _map(97, 63, holes=False)
    yy, xx = np.mgrid[0:63, 0:97]
    smooth = (4.0 + 0.02 * np.abs(xx - 40.0) + 0.01 * np.abs(yy - 30.0)).astype(np.float32)
    free = simplify_ref.triangulate(smooth)
    assert 4 < free["iterations"] < 97 * 63 // 40
    stop = free["iterations"]
    cases = [(smooth, stop - 3, -1.0), (smooth, stop + 50, -1.0), (smooth, -1, 0.0),
             (smooth, -1, 1e-4), (smooth, -1, 0.5), (dm, 0, -1.0), (dm, 1, -1.0),
             (dm, 400, -1.0), (dm, -1, 0.02)]
    for i, (m, mv, me) in enumerate(cases):
        got = hip.simplify_triangulate(m, max_vertices=mv, max_error=me)
        want = simplify_ref.triangulate(m, max_vertices=mv, max_error=me)
        _assert_same_triangulation(got, want, "bounds-%d" % i)
    assert simplify_ref.triangulate(smooth, stop - 3)["iterations"] == stop - 3
    assert simplify_ref.triangulate(smooth, stop + 50)["iterations"] == stop


def test_triangulation_of_degenerate_maps(hip):
    """An all-zero map inserts (0, 0, 0) once and idles through its budget
    (S2 / S5 / S7); constant maps follow the rows, whatever their float sum."""
    zero = np.zeros((20, 30), np.float32)
    got = hip.simplify_triangulate(zero)
    assert got["iterations"] == 15 and len(got["vertices"]) == 5
    assert np.array_equal(got["vertices"][4], [0.0, 0.0, 0.0])
    _assert_same_triangulation(got, simplify_ref.triangulate(zero), "zero")
    for shape, value in (((8, 8), 2.0), ((40, 40), 2.0), ((40, 40), 0.1), ((33, 47), 3.7)):
        const = np.full(shape, value, np.float32)
        _assert_same_triangulation(hip.simplify_triangulate(const),
                                   simplify_ref.triangulate(const),
                                   "const-%dx%d-%g" % (shape[1], shape[0], value))


def _inputs(n_views, w, h, channels, seed=5):
    from smvs_amd import synth
    inputs = synth.pipeline_inputs("sphere", w, h, max(n_views - 1, 1), flen=1.2)
    cams = inputs["cams"][:n_views]
    depths, normals = synth.depth_and_normal_maps(inputs["scene"], cams)
    rng = np.random.default_rng(seed)
    for i in range(n_views):
        depths[i] *= (1.0 + 0.002 * rng.standard_normal(depths[i].shape)).astype(np.float32)
        depths[i][rng.random(depths[i].shape) < 0.01] = 0.0
    depths[0][h // 5:h // 5 + 9, w // 4:w // 4 + 13] = 0.0
    images = [rng.integers(0, 256, (h, w) if channels == 1 else (h, w, channels))
              .astype(np.uint8) for _ in range(n_views)]
    return cams, depths, normals, images


def _cut_maps(oracle, cams, depths, normals, cut):
    if cut and len(cams) > 1:
        return oracle.cut_depth_maps(cams, depths, normals)
    dms, wn = [], []
    for c, d, n in zip(cams, depths, normals):
        a, b = oracle.cut_depth_maps([c], [d], [n])
        dms.append(a[0])
        wn.append(b[0])
    return dms, wn


def _assert_same_export(got, want, mesh, label):
    assert len(got["xyz"]) == len(want["xyz"]) > 0
    exact = ["xyz", "rgb", "confidence"]
    if "faces" in want:
        assert len(got["faces"]) == len(want["faces"]) > 0
        exact.append("faces")
    else:
        assert "faces" not in got
    if not mesh:
        exact += ["value", "normals"]
    else:
        assert "value" not in got
    for k in exact:
        assert np.array_equal(got[k], want[k]), k
    if mesh:
        d = np.abs(got["normals"].astype(np.float64) - want["normals"])
        print("SIMPLIFY_NORMALS %s vertices=%d faces=%d max_abs_diff=%.3g differing=%d"
              % (label, len(got["xyz"]), len(got["faces"]), d.max(),
                 int((d.max(axis=1) > 0).sum())))
        assert d.max() <= NORMAL_TOL
        assert np.array_equal(np.all(got["normals"] == 0, axis=1),
                              np.all(want["normals"] == 0, axis=1))
    else:
        print("SIMPLIFY_POINTS %s vertices=%d confidences=%s"
              % (label, len(got["xyz"]), np.unique(got["confidence"]).tolist()))


@pytest.mark.parametrize("mesh", [False, True])
@pytest.mark.parametrize("n_views,w,h,channels,cut", [
    (1, 96, 64, 3, True), (2, 97, 63, 1, True), (2, 97, 63, 3, False),
    (9, 161, 121, 3, True), (9, 161, 121, 1, False)])
def test_export_matches_restatement(hip, oracle, n_views, w, h, channels, cut, mesh):
    cams, depths, normals, images = _inputs(n_views, w, h, channels)
    got = hip.generate_simplified(cams, depths, normals, images, mesh=mesh, cut=cut,
                                  cut_maps=True)
    dms, wn = _cut_maps(oracle, cams, depths, normals, cut)
    want = simplify_ref.simplified(cams, dms, wn, images, mesh=mesh)
    for a, b in zip(got["cut_depth"], dms):
        assert np.array_equal(a, b)
    _assert_same_export(got, want, mesh, "%dx%dx%d-c%d-cut%d-mesh%d"
                        % (n_views, w, h, channels, cut, mesh))
    assert got["faces"].max() < len(got["xyz"])
    assert len(np.unique(got["confidence"])) >= 2   # border vertices and others


@pytest.mark.parametrize("mesh", [False, True])
def test_export_with_aabb_and_bounds(hip, oracle, mesh):
    cams, depths, normals, images = _inputs(3, 161, 121, 3)
    dms, wn = _cut_maps(oracle, cams, depths, normals, True)
    full = simplify_ref.simplified(cams, dms, wn, images, mesh=False)
    lo = np.percentile(full["xyz"], 20, axis=0).astype(np.float32)
    hi = np.percentile(full["xyz"], 85, axis=0).astype(np.float32)
    got = hip.generate_simplified(cams, depths, normals, images, mesh=mesh, aabb=(lo, hi))
    want = simplify_ref.simplified(cams, dms, wn, images, mesh=mesh, aabb=(lo, hi))
    assert 0 < len(want["xyz"]) < len(full["xyz"])
    _assert_same_export(got, want, mesh, "aabb-mesh%d" % mesh)
    got = hip.generate_simplified(cams, depths, normals, images, mesh=mesh,
                                  max_vertices=150, max_error=0.004)
    want = simplify_ref.simplified(cams, dms, wn, images, mesh=mesh, max_vertices=150,
                                   max_error=0.004)
    _assert_same_export(got, want, mesh, "bounds-mesh%d" % mesh)


@pytest.mark.parametrize("mesh", [False, True])
def test_export_box_around_everything_changes_nothing(hip, mesh):
    """The shared AABB clip with a box that holds every vertex (the unclipped
    min / max, one float step outward): bit for bit the unclipped export; the
    point cloud's faces are not returned together with a box."""
    cams, depths, normals, images = _inputs(3, 128, 96, 3)
    full = hip.generate_simplified(cams, depths, normals, images, mesh=mesh)
    lo = np.nextafter(full["xyz"].min(axis=0), np.float32(-np.inf))
    hi = np.nextafter(full["xyz"].max(axis=0), np.float32(np.inf))
    got = hip.generate_simplified(cams, depths, normals, images, mesh=mesh, aabb=(lo, hi))
    keys = ["xyz", "normals", "rgb", "confidence"] + (["faces"] if mesh else ["value"])
    assert sorted(got) == sorted(keys)
    assert len(got["xyz"]) > 0
    for k in keys:
        assert got[k].dtype == full[k].dtype and got[k].shape == full[k].shape, k
        assert got[k].tobytes() == full[k].tobytes(), k


def test_view_without_valid_depth_contributes_nothing(hip, oracle):
    cams, depths, normals, images = _inputs(3, 97, 63, 3)
    depths[1][:] = 0.0
    got = hip.generate_simplified(cams, depths, normals, images, cut=False)
    dms, wn = _cut_maps(oracle, cams, depths, normals, False)
    want = simplify_ref.simplified(cams, dms, wn, images)
    _assert_same_export(got, want, False, "empty-view")
    two = hip.generate_simplified([cams[0], cams[2]], [depths[0], depths[2]],
                                  [normals[0], normals[2]], [images[0], images[2]], cut=False)
    assert np.array_equal(two["xyz"], got["xyz"]) and np.array_equal(two["faces"], got["faces"])


def test_simplified_rejects_bad_arguments(hip):
    from smvs_amd._capi import SmvsError
    cams, depths, normals, images = _inputs(1, 48, 32, 3)
    for bad in (np.nan, np.inf, -1.0):
        d = depths[0].copy()
        d[5, 7] = bad
        with pytest.raises(SmvsError):
            hip.generate_simplified(cams, [d], normals, images)
        with pytest.raises(SmvsError):
            hip.simplify_triangulate(d)
    with pytest.raises(SmvsError):
        hip.simplify_triangulate(np.ones((1, 40), np.float32))
    with pytest.raises(SmvsError):
        hip.simplify_triangulate(np.ones((2, 4097), np.float32))
    with pytest.raises(SmvsError):
        hip.simplify_triangulate(depths[0], max_vertices=-2)
    with pytest.raises(SmvsError):
        hip.simplify_triangulate(depths[0], max_error=-0.5)
    with pytest.raises(ValueError):
        hip.generate_simplified(cams, depths, normals, [images[0][:-1]])


def test_scene_simplified_end_to_end(hip, oracle, tmp_path):
    """mve_scene.write_scene -> host.reconstruct_scene (3 views) ->
    host.generate_simplified for both outputs: smvs-B0.ply and smvs-m-B0.ply,
    their contents equal to the restatement on the saved embeddings."""
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
    dms, wn = _cut_maps(oracle, cams, depths, normals, True)
    for mesh, name in ((False, "smvs-B0.ply"), (True, "smvs-m-B0.ply")):
        path, nv, nf = host.generate_simplified(d, mesh=mesh, input_scale=0)
        assert os.path.basename(path) == name and os.path.dirname(path) == d
        want = simplify_ref.simplified(cams, dms, wn, images, mesh=mesh)
        if mesh:
            lines, props, faces = mesh_ref.read_ply_mesh(path)
            assert "element face %d" % nf in lines and nf == len(want["faces"])
        else:
            props, names, _, rest = points_ref.read_ply(path)
            assert "value" in names and rest == 0
            want = {k: v for k, v in want.items() if k != "faces"}
        got = {"xyz": np.stack([props["x"], props["y"], props["z"]], 1),
               "normals": np.stack([props["nx"], props["ny"], props["nz"]], 1),
               "rgb": np.stack([props["red"], props["green"], props["blue"]], 1),
               "confidence": props["confidence"]}
        if mesh:
            got["faces"] = faces.astype(np.uint32)
        else:
            got["value"] = props["value"]
        assert nv == len(want["xyz"])
        _assert_same_export(got, want, mesh, "scene-mesh%d" % mesh)
    for v, c in zip(vdirs, dms):
        assert np.array_equal(mve_scene.load_mvei(os.path.join(v, "smvs-cut.mvei")), c)
