"""smvs_points_generate (the point cloud of MeshGenerator::generate_mesh on
the device) against the serial CPU restatement tests/points_reference.cc run
on the oracle's cut maps: positions, colours, normals, confidences, scale
values, faces and the vertex order identical."""
import os

import numpy as np
import pytest

import points_ref  # tests/points_ref.py

pytestmark = pytest.mark.gpu

KEYS = ("xyz", "normals", "rgb", "confidence", "value")


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


def _reference(oracle, cams, depths, normals, images, cut, aabb=None):
    if cut and len(cams) > 1:
        dms, wn = oracle.cut_depth_maps(cams, depths, normals)
    else:
        dms, wn = [], []
        for c, d, n in zip(cams, depths, normals):
            a, b = oracle.cut_depth_maps([c], [d], [n])
            dms.append(a[0])
            wn.append(b[0])
    return points_ref.points(cams, dms, wn, images, aabb=aabb), dms


def _assert_same(got, want, faces=True):
    assert len(got["xyz"]) == len(want["xyz"]) > 0
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), k
    if faces:
        assert np.array_equal(got["faces"], want["faces"])


@pytest.mark.parametrize("n_views,w,h,channels,cut", [
    (1, 96, 64, 3, True), (2, 97, 63, 1, True), (2, 97, 63, 3, False),
    (9, 161, 121, 3, True), (9, 161, 121, 1, False)])
def test_points_match_restatement(hip, oracle, n_views, w, h, channels, cut):
    _, cams, depths, normals, images = _inputs(n_views, w, h, channels)
    got = hip.generate_points(cams, depths, normals, images, cut=cut, faces=True,
                              cut_maps=True)
    want, dms = _reference(oracle, cams, depths, normals, images, cut)
    _assert_same(got, want)
    for a, b in zip(got["cut_depth"], dms):
        assert np.array_equal(a, b)
    assert set(np.unique(got["confidence"]).tolist()) <= {0.0, 0.25, 0.5, 0.75, 1.0}
    if cut and n_views > 1:
        plain = hip.generate_points(cams, depths, normals, images, cut=False)
        assert len(plain["xyz"]) > len(got["xyz"])


@pytest.mark.parametrize("cut", [True, False])
def test_points_aabb_clip(hip, oracle, cut):
    _, cams, depths, normals, images = _inputs(3, 128, 96, 3, seed=8)
    aabb = ((-0.6, -0.5, 0.0), (0.7, 0.6, 4.5))
    got = hip.generate_points(cams, depths, normals, images, cut=cut, aabb=aabb)
    want, _ = _reference(oracle, cams, depths, normals, images, cut, aabb=aabb)
    _assert_same(got, want, faces=False)
    full = hip.generate_points(cams, depths, normals, images, cut=cut)
    assert 0 < len(got["xyz"]) < len(full["xyz"])


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_points_box_around_everything_changes_nothing(hip):
    """The shared AABB clip with a box that holds every vertex (the unclipped
    min / max, one float step outward): bit for bit the unclipped cloud."""
    _, cams, depths, normals, images = _inputs(3, 128, 96, 3, seed=8)
    full = hip.generate_points(cams, depths, normals, images, cut=True)
    assert len(full["xyz"]) > 4096          # more than one scan tile
    lo = np.nextafter(full["xyz"].min(axis=0), np.float32(-np.inf))
    hi = np.nextafter(full["xyz"].max(axis=0), np.float32(np.inf))
    got = hip.generate_points(cams, depths, normals, images, cut=True, aabb=(lo, hi))
    for k in KEYS:
        assert _same_bits(got[k], full[k]), k


def test_points_aabb_clip_keeps_the_merged_order(hip):
    """The clipped cloud is the unclipped one filtered by the inclusive box
    test, in the unclipped order, across the scan's 4096-element tiles."""
    _, cams, depths, normals, images = _inputs(3, 128, 96, 3, seed=8)
    aabb = ((-0.6, -0.5, 0.0), (0.7, 0.6, 4.5))
    full = hip.generate_points(cams, depths, normals, images, cut=True)
    got = hip.generate_points(cams, depths, normals, images, cut=True, aabb=aabb)
    lo, hi = np.float32(aabb[0]), np.float32(aabb[1])
    keep = ~((full["xyz"] < lo) | (full["xyz"] > hi)).any(axis=1)
    assert len(full["xyz"]) > 2 * 4096 and 0 < keep.sum() < len(keep)
    # kept and dropped vertices in more than one tile each
    tiles = np.arange(len(keep)) // 4096
    assert len(np.unique(tiles[keep])) > 1 and len(np.unique(tiles[~keep])) > 1
    for k in KEYS:
        assert _same_bits(got[k], full[k][keep]), k


def test_points_full_size_nine_views(hip, oracle):
    scene, cams, depths, normals, images = _inputs(9, 1920, 1080, 3, seed=11)
    got = hip.generate_points(cams, depths, normals, images, cut=True, faces=True)
    want, _ = _reference(oracle, cams, depths, normals, images, True)
    _assert_same(got, want)


def test_points_lie_on_the_synthetic_surfaces(hip):
    from smvs_amd import synth
    inputs = synth.pipeline_inputs("sphere", 320, 240, 4, flen=1.2)
    cams = inputs["cams"]
    depths, normals = synth.depth_and_normal_maps(inputs["scene"], cams)
    images = [np.zeros((240, 320), np.uint8) for _ in cams]
    got = hip.generate_points(cams, depths, normals, images, cut=False)
    X = got["xyz"].astype(np.float64)
    scene = inputs["scene"]
    r = np.abs(np.linalg.norm(X - scene.c, axis=1) - scene.r)
    plane = np.abs(X[:, 2] - scene.plane_z)
    dist = np.minimum(r, plane)
    depth = np.linalg.norm(X - cams[0].center, axis=1)
    assert len(X) > 0.9 * 240 * 320 * len(cams)
    assert np.all(dist <= 2e-6 * depth + 1e-6)


def test_points_reject_bad_arguments(hip):
    from smvs_amd._capi import SmvsError
    _, cams, depths, normals, images = _inputs(2, 64, 48, 3)
    with pytest.raises(SmvsError):
        hip.generate_points([], [], [], [])
    with pytest.raises(SmvsError):
        hip.generate_points(cams, depths, normals, images, dd_factor=-1.0)
    with pytest.raises(SmvsError):
        hip.generate_points(cams, depths, normals, images, aabb=((0, 0, 0), (1, 1, 1)),
                            faces=True)
    with pytest.raises(ValueError):
        hip.generate_points(cams, depths, normals, [images[0][:10]] * 2)


def test_scene_point_cloud_end_to_end(hip, oracle, tmp_path):
    """mve_scene.write_scene -> host.reconstruct_scene (3 views) ->
    host.generate_point_cloud: smvsrecon's .ply name, its vertices equal to
    the restatement on the saved embeddings, smvs-cut.mvei equal to
    smvs_cut_depth_maps' output; --mesh / --simplify refused."""
    from smvs_amd import synth, host, mve_scene
    from smvs_amd._capi import SmvsError
    inputs = synth.pipeline_inputs("sphere", 192, 128, 2, flen=1.2)
    d = str(tmp_path)
    mve_scene.write_scene(d, inputs)
    done, _, _ = host.reconstruct_scene(d, view_ids=[0, 1, 2], num_neighbors=2,
                                        min_neighbors=1, output_scale=2, input_scale=0)
    assert sorted(done) == [0, 1, 2]
    path, n = host.generate_point_cloud(d, input_scale=0)
    assert os.path.basename(path) == "smvs-B0.ply" and os.path.dirname(path) == d
    props, names, n_faces, rest = points_ref.read_ply(path)
    assert names == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue",
                     "confidence", "value"]
    assert n_faces == 0 and rest == 0 and len(props["x"]) == n > 0
    cams = inputs["cams"][:3]
    vdirs = [os.path.join(d, "views", "view_%04d.mve" % i) for i in range(3)]
    depths = [mve_scene.load_mvei(os.path.join(v, "smvs-B0.mvei")) for v in vdirs]
    normals = [mve_scene.load_mvei(os.path.join(v, "smvs-B0N.mvei")) for v in vdirs]
    images = [mve_scene.load_mvei(os.path.join(v, "undistorted.mvei")) for v in vdirs]
    want, _ = _reference(oracle, cams, depths, normals, images, True)
    assert np.array_equal(np.stack([props["x"], props["y"], props["z"]], 1), want["xyz"])
    assert np.array_equal(np.stack([props["nx"], props["ny"], props["nz"]], 1),
                          want["normals"])
    assert np.array_equal(np.stack([props["red"], props["green"], props["blue"]], 1),
                          want["rgb"])
    assert np.array_equal(props["confidence"], want["confidence"])
    assert np.array_equal(props["value"], want["value"])
    cut_d, _ = hip.cut_depth_maps(cams, depths, normals)
    for v, c in zip(vdirs, cut_d):
        assert np.array_equal(mve_scene.load_mvei(os.path.join(v, "smvs-cut.mvei")), c)
    with pytest.raises(SmvsError):
        host.generate_point_cloud(d, input_scale=0, mesh=True)
    with pytest.raises(SmvsError):
        host.generate_point_cloud(d, input_scale=0, simplify=True)
