"""smvs_tsdf_fuse / smvs_tsdf_bounds on the device against the numpy
restatement of their definition (tests/tsdf_ref.py), run on the oracle's cut
maps: the whole volume (NaN positions included), the weights, and every
attribute of the mesh are equal to the bit, and the faces and their order are
the same."""
import os

import numpy as np
import pytest

import mesh_ref  # tests/mesh_ref.py
import tsdf_ref  # tests/tsdf_ref.py

pytestmark = pytest.mark.gpu

KEYS = ("weight", "xyz", "normals", "rgb", "confidence", "faces")
DIMS = (37, 29, 23)          # no dimension a multiple of a brick or block side
VOXEL = 0.06
SURFACE_BOX = (-1.1, -0.9, 2.8)      # around the sphere's visible front (z = 3)


@pytest.fixture(scope="module")
def hip():
    import smvs_amd
    if smvs_amd.device_count() < 1:
        pytest.fail("no HIP device")
    return smvs_amd


def _inputs(n_views, w, h, channels, seed=5, last_size=None):
    """The views of test_gpu_mesh.py's _inputs (1 % holes, noise, a depth step
    in view 0); with last_size the last view has a size of its own."""
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


def _compare(hip, oracle, cams, depths, normals, images, origin, voxel, dims, cut, label,
             **kw):
    got = hip.fuse_tsdf(cams, depths, normals, images, origin, voxel, dims, cut=cut,
                        volume=True, **kw)
    dms = _cut_maps(oracle, cams, depths, normals, cut)
    want = tsdf_ref.fuse(cams, dms, images, origin, voxel, dims, **kw)
    unknown = np.isnan(want["tsdf"])
    print("TSDF %s voxels=%d unknown=%d vertices=%d faces=%d (device %d, %d)"
          % (label, unknown.size, unknown.sum(), len(want["xyz"]), len(want["faces"]),
             len(got["xyz"]), len(got["faces"])))
    assert np.array_equal(np.isnan(got["tsdf"]), unknown)
    assert np.array_equal(got["tsdf"], want["tsdf"], equal_nan=True)
    for k in KEYS:
        assert got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k]), k
    assert set(got) == set(want)
    return got


def _boundary_edges(faces):
    f = faces.astype(np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    e.sort(axis=1)
    _, counts = np.unique(e, axis=0, return_counts=True)
    assert counts.max() <= 2
    return int((counts == 1).sum())


@pytest.mark.parametrize("n_views,channels,cut,min_weight", [
    (1, 3, True, 1), (2, 1, True, 1), (2, 3, False, 2), (5, 3, True, 2), (5, 1, False, 1)])
def test_fusion_matches_restatement(hip, oracle, n_views, channels, cut, min_weight):
    cams, depths, normals, images = _inputs(n_views, 97, 63, channels)
    got = _compare(hip, oracle, cams, depths, normals, images, SURFACE_BOX, VOXEL, DIMS, cut,
                   "%dv-c%d-cut%d-mw%d" % (n_views, channels, cut, min_weight),
                   min_weight=min_weight)
    assert len(got["faces"]) > 100 and got["faces"].max() < len(got["xyz"])


def test_a_view_of_another_size_and_an_explicit_truncation(hip, oracle):
    cams, depths, normals, images = _inputs(3, 97, 63, 3, last_size=(80, 71))
    assert depths[2].shape == (71, 80) != depths[0].shape
    got = _compare(hip, oracle, cams, depths, normals, images, SURFACE_BOX, VOXEL, DIMS, True,
                   "mixed-sizes", trunc=0.1)
    assert len(got["faces"]) > 100


def test_two_cubed(hip, oracle):
    # one cell across the sphere's front: at most one vertex, never a face
    cams, depths, normals, images = _inputs(2, 97, 63, 3)
    got = _compare(hip, oracle, cams, depths, normals, images, (-0.06, -0.06, 2.95), VOXEL,
                   (2, 2, 2), False, "2x2x2")
    assert len(got["xyz"]) == 1 and len(got["faces"]) == 0


def test_box_around_a_camera_centre(hip, oracle):
    # voxels behind and on the cameras' planes (proj[2] <= 0) and the surface
    cams, depths, normals, images = _inputs(5, 97, 63, 1)
    origin, voxel, dims = (-0.6, -0.5, -0.62), 0.15, (8, 7, 41)
    centre = np.asarray(cams[1].center)
    assert np.all(centre > origin) and np.all(centre < np.asarray(origin) + voxel * np.array(dims))
    got = _compare(hip, oracle, cams, depths, normals, images, origin, voxel, dims, True,
                   "camera-inside")
    behind = got["weight"][:4]          # z < 0: behind every camera
    assert np.all(behind == 0) and np.all(np.isnan(got["tsdf"][:4]))
    assert len(got["faces"]) > 0


def test_box_half_outside_every_frustum(hip, oracle):
    cams, depths, normals, images = _inputs(5, 97, 63, 3)
    got = _compare(hip, oracle, cams, depths, normals, images, (-1.0, -0.2, 2.8), VOXEL, DIMS,
                   True, "half-outside")
    unknown = np.isnan(got["tsdf"])
    assert unknown[:, -3:, :].all() and not unknown[:, :8, :].all()
    assert len(got["faces"]) > 100
    assert _boundary_edges(got["faces"]) > 0       # an open mesh boundary


def test_box_away_from_the_surface(hip, oracle):
    cams, depths, normals, images = _inputs(2, 97, 63, 3)
    got = _compare(hip, oracle, cams, depths, normals, images, (-0.3, -0.2, 1.0), 0.03,
                   (9, 8, 7), True, "free-space")
    assert got["xyz"].shape == (0, 3) and got["faces"].shape == (0, 3)
    assert got["weight"].max() > 0 and np.nanmin(got["tsdf"]) == 1.0


@pytest.mark.parametrize("n_views,cut", [(1, True), (3, True), (3, False)])
def test_bounds(hip, oracle, n_views, cut):
    cams, depths, normals, _ = _inputs(n_views, 97, 63, 1, last_size=(80, 71))
    lo, hi = hip.tsdf_bounds(cams, depths, normals, cut=cut)
    dms = _cut_maps(oracle, cams, depths, normals, cut)
    want_lo, want_hi = tsdf_ref.bounds(cams, dms)
    pts = np.concatenate([tsdf_ref.world_points(tsdf_ref.camera(c, d.shape[1], d.shape[0]), d)
                          for c, d in zip(cams, dms)])
    assert np.array_equal(want_lo, pts.min(axis=0)) and np.array_equal(want_hi, pts.max(axis=0))
    assert np.array_equal(lo, want_lo) and np.array_equal(hi, want_hi)
    assert np.all(lo < hi)
    if not cut:
        # the normals are not needed without the cut
        lo2, hi2 = hip.tsdf_bounds(cams, depths, None, cut=False)
        assert np.array_equal(lo2, lo) and np.array_equal(hi2, hi)


def test_bounds_without_a_valid_pixel(hip):
    cams, depths, normals, _ = _inputs(2, 97, 63, 1)
    lo, hi = hip.tsdf_bounds(cams, [np.zeros_like(d) for d in depths], normals, cut=True)
    assert np.all(lo > hi)
    assert np.all(np.isposinf(lo)) and np.all(np.isneginf(hi))


def test_no_normals_without_the_cut_and_refusals(hip, oracle):
    from smvs_amd._capi import SmvsError
    cams, depths, normals, images = _inputs(2, 97, 63, 3)
    a = hip.fuse_tsdf(cams, depths, None, images, SURFACE_BOX, VOXEL, DIMS, cut=False)
    b = hip.fuse_tsdf(cams, depths, normals, images, SURFACE_BOX, VOXEL, DIMS, cut=False)
    assert set(a) == {"xyz", "normals", "rgb", "confidence", "faces"}
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    with pytest.raises(SmvsError):
        hip.fuse_tsdf(cams, depths, None, images, SURFACE_BOX, VOXEL, DIMS, cut=True)
    with pytest.raises(SmvsError):
        hip.fuse_tsdf(cams, depths, normals, images, SURFACE_BOX, 0.0, DIMS)
    with pytest.raises(SmvsError):
        hip.fuse_tsdf(cams, depths, normals, images, SURFACE_BOX, VOXEL, (37, 1, 23))
    # the mesh export next to it still gives what it gave
    m = hip.generate_mesh(cams, depths, normals, images, cut=True)
    dms, wn = oracle.cut_depth_maps(cams, depths, normals)
    want = mesh_ref.mesh(cams, dms, wn, images)
    for k in ("xyz", "rgb", "confidence", "faces"):
        assert np.array_equal(m[k], want[k]), k


def test_scene_fused_end_to_end(hip, tmp_path):
    """mve_scene.write_scene -> host.reconstruct_scene (3 views) ->
    host.generate_fused: smvs-fused-B0.ply holds what the C ABI gives for the
    saved embeddings and the same box."""
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

    def read(path, nv, nf):
        lines, props, faces = mesh_ref.read_ply_mesh(path)
        assert "element vertex %d" % nv in lines and "element face %d" % nf in lines
        assert "property float value" not in lines
        return {"xyz": np.stack([props["x"], props["y"], props["z"]], 1),
                "normals": np.stack([props["nx"], props["ny"], props["nz"]], 1),
                "rgb": np.stack([props["red"], props["green"], props["blue"]], 1),
                "confidence": props["confidence"], "faces": faces.astype(np.uint32)}

    # an explicit box and voxel size
    lo, hi = np.float32((-1.0, -0.8, 2.8)), np.float32((1.0, 0.8, 4.3))
    voxel = np.float32(0.05)
    path, nv, nf = host.generate_fused(d, voxel_size=voxel, aabb=(lo, hi), input_scale=0)
    assert os.path.basename(path) == "smvs-fused-B0.ply" and os.path.dirname(path) == d
    dims = [max(2, int(np.ceil((hi[a] - lo[a]) / voxel))) for a in range(3)]
    want = hip.fuse_tsdf(cams, depths, normals, images, lo, voxel, dims, cut=True)
    got = read(path, nv, nf)
    assert nf > 100
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    # the defaults: the bounds padded by 3 voxels, the longest side / resolution
    path, nv, nf = host.generate_fused(d, resolution=64, input_scale=0)
    blo, bhi = hip.tsdf_bounds(cams, depths, normals, cut=True)
    voxel = np.float32((bhi - blo).max() / np.float32(64 - 6))
    pad = np.float32(3.0) * voxel
    lo, hi = blo - pad, bhi + pad
    dims = [max(2, int(np.ceil((hi[a] - lo[a]) / voxel))) for a in range(3)]
    assert max(dims) in (64, 65)
    want = hip.fuse_tsdf(cams, depths, normals, images, lo, voxel, dims, cut=True)
    got = read(path, nv, nf)
    assert nf > 100
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    # the exports next to it are not touched by the fusion
    assert not os.path.exists(os.path.join(vdirs[0], "smvs-cut.mvei"))
