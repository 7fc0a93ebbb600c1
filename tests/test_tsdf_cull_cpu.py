"""The brick cull's definition (tests/tsdf_cull_ref.py, the comment of
smvs_tsdf_fuse_sparse_opts in include/smvs_hip.h) on the CPU: the pyramid
against a brute-force min / max, candidate >= seed brick with no miss on every
box the device tests use and on random boxes and poses, the effectiveness the
cull is built for, the fusion over the candidates alone, and the refusals of
the Python layer.  No GPU."""
import numpy as np
import pytest

import tsdf_cull_cases as cases  # tests/tsdf_cull_cases.py
import tsdf_cull_ref  # tests/tsdf_cull_ref.py
import tsdf_ref  # tests/tsdf_ref.py
import tsdf_sparse_ref  # tests/tsdf_sparse_ref.py

f32 = np.float32


# -------------------------------------------------------------------- pyramid
def _map(w, h, seed):
    rng = np.random.default_rng(seed)
    D = (1.0 + rng.random((h, w))).astype(f32)
    D[rng.random((h, w)) < 0.3] = 0.0
    return D


@pytest.mark.parametrize("w,h", [(97, 63), (80, 71), (5, 3), (1, 7), (1, 1)])
def test_pyramid_is_the_min_max_over_each_texels_pixels(w, h):
    D = _map(w, h, 7 * w + h)
    levels = tsdf_cull_ref.pyramid(D)
    n = max(w, h)
    assert len(levels) == 1 + int(np.ceil(np.log2(n))) if n > 1 else len(levels) == 1
    assert levels[-1][0].shape == (1, 1)
    for l, (lo, hi) in enumerate(levels):
        assert lo.shape == hi.shape == (-(-h // (1 << l)), -(-w // (1 << l)))
        assert lo.dtype == hi.dtype == f32
        blo, bhi = tsdf_cull_ref.pyramid_brute(D, l)
        assert np.array_equal(lo, blo) and np.array_equal(hi, bhi), l
    valid = D != 0
    if valid.any():
        assert levels[-1][0][0, 0] == D[valid].min() and levels[-1][1][0, 0] == D[valid].max()


def test_pyramid_of_an_all_invalid_map_and_of_one_valid_pixel():
    D = np.zeros((63, 97), f32)
    for lo, hi in tsdf_cull_ref.pyramid(D):
        assert np.all(lo == np.inf) and np.all(hi == -np.inf)
    D[40, 71] = f32(2.5)
    D[3, 3] = f32(np.nan)           # NaN passes no step of the field either
    for l, (lo, hi) in enumerate(tsdf_cull_ref.pyramid(D)):
        want = np.zeros(lo.shape, bool)
        want[40 >> l, 71 >> l] = True
        assert np.array_equal(lo == f32(2.5), want) and np.array_equal(hi == f32(2.5), want)
        assert np.all(lo[~want] == np.inf) and np.all(hi[~want] == -np.inf)


# ------------------------------------------------------------ candidate >= seed
def _seed_and_candidates(cams, maps, images, box, trunc=0):
    origin, voxel, dims = box
    _, _, col = tsdf_ref.field(cams, maps, images, origin, voxel, dims, trunc)
    bx, by, bz = tsdf_sparse_ref.brick_dims(dims)
    seed = tsdf_sparse_ref._seed_bricks(col[..., 3], (bz, by, bx))
    cand = tsdf_cull_ref.candidates(cams, maps, origin, voxel, dims, trunc)
    assert cand.shape == seed.shape and cand.dtype == np.uint8
    return seed, cand != 0


@pytest.fixture(scope="module")
def five():
    cams, depths, normals, images = cases.inputs(5)
    for d in depths:
        d.setflags(write=False)
    return cams, depths, normals, images


@pytest.fixture(scope="module")
def counted(five):
    """label -> (bricks, seed bricks, candidates, missed) of the table's boxes"""
    cams, depths, _, images = five
    rows = [("small", cases.SMALL, 5, 0), ("deep", cases.DEEP, 5, 0),
            ("deep-trunc", cases.DEEP, 5, 0.1), ("free", cases.FREE, 2, 0),
            ("half-outside", cases.HALF_OUTSIDE, 5, 0),
            ("around-camera", cases.AROUND_CAMERA, 5, 0), ("bar", cases.BAR, 2, 0),
            ("fine", cases.FINE, 5, 0)]
    out = {}
    for label, box, n, trunc in rows:
        seed, cand = _seed_and_candidates(cams[:n], depths[:n], images[:n], box, trunc)
        out[label] = (seed.size, int(seed.sum()), int(cand.sum()), int((seed & ~cand).sum()))
        print("TSDF-CULL-CPU %-14s bricks=%d seed=%d candidates=%d missed=%d"
              % ((label,) + out[label]))
    return out


@pytest.mark.parametrize("label", ["small", "deep", "deep-trunc", "free", "half-outside",
                                   "around-camera", "bar", "fine"])
def test_no_seed_brick_is_culled(counted, label):
    bricks, seed, cand, missed = counted[label]
    assert missed == 0
    assert seed <= cand <= bricks
    if label != "free":
        assert seed > 0


def test_the_cull_is_effective(counted):
    assert 3 * counted["deep"][2] <= counted["deep"][0]
    assert 5 * counted["fine"][2] <= counted["fine"][0]
    assert counted["free"][2] == 0


def test_shifted_world():
    shift = (500.0, -300.0, 200.0)
    cams, depths, _, images = cases.inputs(3, shift=shift)
    origin = tuple(o + s for o, s in zip(cases.DEEP[0], shift))
    seed, cand = _seed_and_candidates(cams, depths, images, (origin,) + cases.DEEP[1:])
    assert seed.sum() > 50 and not (seed & ~cand).any()
    assert 3 * cand.sum() <= cand.size


@pytest.mark.parametrize("box", [cases.SMALL, cases.DEEP], ids=["small", "deep"])
def test_cut_maps_from_the_oracle(oracle, five, box):
    cams, depths, normals, images = five
    cut = oracle.cut_depth_maps(cams, depths, normals)[0]
    assert any(not np.array_equal(c, d) for c, d in zip(cut, depths))
    seed, cand = _seed_and_candidates(cams, cut, images, box)
    assert seed.sum() > 20 and not (seed & ~cand).any()


@pytest.mark.parametrize("box", [cases.SMALL, cases.DEEP], ids=["small", "deep"])
def test_a_view_of_another_size(box):
    cams, depths, _, images = cases.inputs(3, last_size=(80, 71))
    assert depths[2].shape == (71, 80)
    seed, cand = _seed_and_candidates(cams, depths, images, box, 0.1)
    assert seed.sum() > 20 and not (seed & ~cand).any()
    # the odd view alone
    seed, cand = _seed_and_candidates(cams[2:], depths[2:], images[2:], box, 0.1)
    assert seed.sum() > 20 and not (seed & ~cand).any()


@pytest.mark.parametrize("roll", [0.6, np.pi / 2, 2.5])
def test_a_rolled_camera(roll):
    cams, depths, _, images = cases.inputs(2, roll=roll)
    seed, cand = _seed_and_candidates(cams[1:], depths[1:], images[1:], cases.DEEP)
    assert seed.sum() > 20 and not (seed & ~cand).any()
    assert 2 * cand.sum() <= cand.size


def test_a_brick_that_straddles_a_cameras_z_0_plane(five):
    """around camera 0 (at the origin, looking along z), 0.15 voxels: the first
    z-slab of bricks has its voxel centres on both sides of that camera's
    z = 0; the view's range there is the whole image"""
    cams, depths, _, images = five
    box = cases.STRADDLE
    lo, hi = tsdf_cull_ref.brick_boxes(*box)
    V = tsdf_ref.camera(cams[0], 97, 63)
    z = [sum(float(V["KR"][6 + k]) * b[k] for k in range(3)) - float(V["t"][2]) for b in (lo, hi)]
    straddle = (np.minimum(*z) < 0) & (np.maximum(*z) > 0)
    assert straddle[0].all() and not straddle[1:].any()
    seed, cand = _seed_and_candidates(cams, depths, images, box)
    assert seed.sum() > 0 and not (seed & ~cand).any()
    # a surface right in front of the camera plane: a map of tiny depths makes
    # the straddling bricks seeds, and they are candidates
    near = [np.full((63, 97), 0.2, f32)]
    seed, cand = _seed_and_candidates(cams[:1], near, images[:1], box)
    assert (seed & straddle).any() and not (seed & ~cand).any()


def test_random_boxes_and_poses():
    from smvs_amd import synth
    rng = np.random.default_rng(2024)
    scene = synth.SphereScene()
    total = missed = 0
    for case in range(30):
        centre = rng.uniform((-2.5, -2.5, -1.0), (2.5, 2.5, 2.0))
        target = rng.uniform((-0.5, -0.5, 3.5), (0.5, 0.5, 4.5))
        R, t = synth.look_at(centre, target)
        roll = rng.uniform(-np.pi, np.pi)
        Rz = np.array([[np.cos(roll), -np.sin(roll), 0.0], [np.sin(roll), np.cos(roll), 0.0],
                       [0.0, 0.0, 1.0]])
        w, h = int(rng.integers(20, 100)), int(rng.integers(20, 100))
        cam = synth.Camera(Rz @ R, Rz @ t, rng.uniform(0.6, 2.0), w, h)
        depths, _ = synth.depth_and_normal_maps(scene, [cam])
        depths[0][rng.random(depths[0].shape) < 0.05] = 0.0
        voxel = rng.uniform(0.02, 0.12)
        dims = tuple(int(x) for x in rng.integers(5, 45, 3))
        # a box around a point the view sees, or anywhere
        seen = tsdf_ref.world_points(tsdf_ref.camera(cam, w, h), depths[0])
        p = seen[rng.integers(len(seen))].astype(float) if case % 3 \
            else rng.uniform((-2.0, -2.0, 0.0), (2.0, 2.0, 6.0))
        origin = tuple(p - rng.uniform(0.2, 0.8, 3) * voxel * np.array(dims))
        images = [np.zeros((h, w), np.uint8)]
        seed, cand = _seed_and_candidates([cam], depths, images, (origin, voxel, dims))
        total += int(seed.sum())
        missed += int((seed & ~cand).sum())
    print("TSDF-CULL-CPU random: seed bricks %d, missed %d" % (total, missed))
    assert missed == 0 and total > 300


# ------------------------------------------------- the fusion on the candidates
@pytest.mark.parametrize("box,min_weight", [(cases.SMALL, 1), (cases.DEEP, 2)],
                         ids=["small-mw1", "deep-mw2"])
def test_fusion_over_the_candidates_is_the_fusion(five, box, min_weight):
    cams, depths, _, images = five
    origin, voxel, dims = box
    want = tsdf_sparse_ref.fuse(cams, depths, images, origin, voxel, dims, min_weight=min_weight)
    cand = tsdf_cull_ref.candidates(cams, depths, origin, voxel, dims)
    got = tsdf_cull_ref.fuse_on_candidates(cams, depths, images, origin, voxel, dims, cand,
                                           min_weight=min_weight)
    assert set(got) == set(want)
    for k in want:
        if k == "stats":
            continue
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k], equal_nan=(k == "tsdf")), k
    tested = got["stats"].pop("tested_bricks")
    assert got["stats"] == want["stats"] and tested == int(cand.sum()) < cand.size
    assert len(want["faces"]) > 100
    # and it is not vacuous: with a seed brick dropped the mesh differs
    worse = cand.copy()
    worse[np.nonzero(want["brick_state"] == 2)[0][0], :, :] = 0
    less = tsdf_cull_ref.fuse_on_candidates(cams, depths, images, origin, voxel, dims, worse,
                                            min_weight=min_weight)
    assert not np.array_equal(less["brick_state"], want["brick_state"])


# ------------------------------------------------------------------- refusals
def test_python_refusals():
    import smvs_amd
    cams, depths, normals, images = cases.inputs(2, 16, 12)
    origin, voxel, dims = cases.SMALL
    with pytest.raises(ValueError):
        smvs_amd.fuse_tsdf(cams, depths, normals, images, origin, voxel, dims, cull=True)
    with pytest.raises(ValueError):
        smvs_amd.fuse_tsdf(cams, depths, normals, images, origin, voxel, dims,
                           brick_candidate=True)
    with pytest.raises(ValueError):
        smvs_amd.fuse_tsdf(cams, depths, normals, images, origin, voxel, dims, sparse=True,
                           brick_candidate=True)
    with pytest.raises(ValueError):
        smvs_amd.tsdf_depth_pyramid(cams, depths, normals, 2)
    from smvs_amd import host
    with pytest.raises(ValueError):
        host.generate_fused("/nonexistent", cull=True)


@pytest.fixture(scope="module")
def lib():
    from smvs_amd import build as hip_build, _capi
    hip_build.build()
    return _capi.load()


def test_entries_refuse_before_any_device_call(lib):
    """status -1 from the three entries on what smvs_tsdf_fuse_sparse refuses;
    no device is touched (this test runs without one)"""
    import ctypes as C
    from smvs_amd import _capi
    from smvs_amd.device import _tsdf_views, _tsdf_options
    cams, depths, normals, images = cases.inputs(2, 16, 12)
    arr, _keep = _tsdf_views(cams, depths, normals, images)
    out = (C.c_uint8 * 4096)()
    good = dict(origin=(-1.0, -1.0, 3.0), voxel_size=0.25, dims=(8, 8, 8), trunc=0.0, cut=True)
    bad = [dict(dims=(8, 1, 8)), dict(dims=(8, 8, 4097)), dict(voxel_size=0.0),
           dict(voxel_size=float("nan")), dict(trunc=float("inf")),
           dict(origin=(0.0, float("nan"), 0.0))]
    for change in bad:
        opt = _tsdf_options(**dict(good, **change))
        assert lib.smvs_tsdf_brick_cull(0, arr, 2, C.byref(opt), out, None) == -1, change
        sopt = _capi.TsdfSparseOpts(0, 1)
        handle = C.c_void_p(1)
        nv, nf = C.c_int64(), C.c_int64()
        assert lib.smvs_tsdf_fuse_sparse_opts(0, arr, 2, C.byref(opt), C.byref(sopt), None,
                                              None, None, None, None, C.byref(handle),
                                              C.byref(nv), C.byref(nf)) == -1, change
        assert handle.value is None
    opt = _tsdf_options(**good)
    assert lib.smvs_tsdf_brick_cull(0, None, 0, C.byref(opt), out, None) == -1
    assert lib.smvs_tsdf_brick_cull(0, arr, 2, C.byref(opt), None, None) == -1
    sopt = _capi.TsdfSparseOpts(1 << 24, 1)
    handle = C.c_void_p(1)
    assert lib.smvs_tsdf_fuse_sparse_opts(0, arr, 2, C.byref(opt), C.byref(sopt), None, None,
                                          None, None, None, C.byref(handle), None, None) == -1
    count, levels = C.c_int64(), C.c_int()
    assert lib.smvs_tsdf_depth_pyramid(0, arr, 2, 1, 2, None, None, C.byref(count),
                                       C.byref(levels)) == -1
    assert lib.smvs_tsdf_depth_pyramid(0, arr, 2, 1, -1, None, None, None, None) == -1
    # the counts alone need no device: 16 x 12 -> 8x6, 4x3, 2x2, 1x1
    assert lib.smvs_tsdf_depth_pyramid(0, arr, 2, 1, 1, None, None, C.byref(count),
                                       C.byref(levels)) == 0
    assert (count.value, levels.value) == (48 + 12 + 4 + 1, 4)
    arr[1].normals = None
    assert lib.smvs_tsdf_brick_cull(0, arr, 2, C.byref(opt), out, None) == -1
