"""The brick cull of the brick-sparse fusion on the device (DESIGN.md section
9.10): fuse_tsdf(sparse=True, cull=True) equals the same call without cull and
tests/tsdf_sparse_ref.py in every array, brick_candidate equals the numpy
restatement of its definition (tests/tsdf_cull_ref.py) to the byte, no seed
brick is culled, and the exact seed test runs on the candidates alone; the
pyramid and the cull through their own entries; the budget; the scene entry."""
import os

import numpy as np
import pytest

import tsdf_cull_cases as cases  # tests/tsdf_cull_cases.py
import tsdf_cull_ref  # tests/tsdf_cull_ref.py
import tsdf_sparse_ref  # tests/tsdf_sparse_ref.py

pytestmark = pytest.mark.gpu

MESH_KEYS = ("xyz", "normals", "rgb", "confidence", "faces")
ALL_KEYS = ("brick_state", "weight") + MESH_KEYS + ("cells",)
SPARSE_STATS = ("bricks", "seed_bricks", "allocated_bricks", "state_bytes")


@pytest.fixture(scope="module")
def hip():
    import smvs_amd
    if smvs_amd.device_count() < 1:
        pytest.fail("no HIP device")
    return smvs_amd


def _cut_maps(oracle, cams, depths, normals, cut):
    if cut and len(cams) > 1:
        return oracle.cut_depth_maps(cams, depths, normals)[0]
    return depths


def _equal(got, want, keys, label):
    for k in keys:
        assert got[k].shape == want[k].shape, (label, k, got[k].shape, want[k].shape)
        assert got[k].dtype == want[k].dtype, (label, k)
        assert np.array_equal(got[k], want[k]), (label, k)


def _check(hip, oracle, cams, depths, normals, images, box, cut, label, **kw):
    """the culled call against the unculled call, the sparse restatement and
    the cull's restatement -> the culled call's dict"""
    origin, voxel, dims = box
    args = (cams, depths, normals, images, origin, voxel, dims)
    got = hip.fuse_tsdf(*args, cut=cut, volume=True, sparse=True, brick_state=True, cull=True,
                        brick_candidate=True, **kw)
    plain = hip.fuse_tsdf(*args, cut=cut, volume=True, sparse=True, brick_state=True, **kw)
    dms = _cut_maps(oracle, cams, depths, normals, cut)
    want = tsdf_sparse_ref.fuse(cams, dms, images, origin, voxel, dims, **kw)
    cand = tsdf_cull_ref.candidates(cams, dms, origin, voxel, dims, kw.get("trunc", 0))
    st = got["stats"]
    print("TSDF-CULL %s bricks=%d seed=%d allocated=%d tested=%d (restatement %d) vertices=%d "
          "faces=%d" % (label, st["bricks"], st["seed_bricks"], st["allocated_bricks"],
                        st["tested_bricks"], int(cand.sum()), len(got["xyz"]),
                        len(got["faces"])))
    assert set(got) == set(plain) | {"brick_candidate"} == set(want) | {"brick_candidate"}
    for other, name in ((plain, "unculled"), (want, "restatement")):
        assert np.array_equal(got["tsdf"], other["tsdf"], equal_nan=True), (label, name)
        _equal(got, other, ALL_KEYS, (label, name))
        assert {k: st[k] for k in SPARSE_STATS} == other["stats"], (label, name)
    assert set(st) == set(SPARSE_STATS) | {"tested_bricks"}
    assert got["brick_candidate"].dtype == np.uint8
    assert np.array_equal(got["brick_candidate"], cand), label
    assert st["tested_bricks"] == int(got["brick_candidate"].sum())
    assert np.all((got["brick_state"] == 2) <= (got["brick_candidate"] != 0)), label
    # the cull through its own entry
    alone = hip.tsdf_brick_cull(cams, depths, normals, origin, voxel, dims,
                                trunc=kw.get("trunc", 0), cut=cut)
    assert alone.dtype == np.uint8 and np.array_equal(alone, got["brick_candidate"]), label
    return got


@pytest.mark.parametrize("box", [cases.SMALL, cases.DEEP], ids=["37x29x23", "61x53x75"])
@pytest.mark.parametrize("n_views,channels,cut,min_weight", [
    (1, 3, True, 1), (3, 1, True, 1), (3, 3, False, 2), (5, 3, True, 2), (5, 1, False, 1)])
def test_culled_fusion_is_the_fusion(hip, oracle, box, n_views, channels, cut, min_weight):
    cams, depths, normals, images = cases.inputs(n_views, channels=channels)
    label = "%s-%dv-c%d-cut%d-mw%d" % (box[2], n_views, channels, cut, min_weight)
    got = _check(hip, oracle, cams, depths, normals, images, box, cut, label,
                 min_weight=min_weight)
    assert len(got["faces"]) > 100
    st = got["stats"]
    assert 0 < st["seed_bricks"] <= st["tested_bricks"] <= st["bricks"]
    if box is cases.DEEP:
        assert 3 * st["tested_bricks"] <= st["bricks"]


@pytest.mark.parametrize("box", [cases.SMALL, cases.DEEP], ids=["37x29x23", "61x53x75"])
def test_a_view_of_another_size_and_an_explicit_truncation(hip, oracle, box):
    cams, depths, normals, images = cases.inputs(3, last_size=(80, 71))
    assert depths[2].shape == (71, 80) != depths[0].shape
    got = _check(hip, oracle, cams, depths, normals, images, box, True, "mixed-sizes", trunc=0.1)
    assert len(got["faces"]) > 100


def test_two_cubed(hip, oracle):
    cams, depths, normals, images = cases.inputs(2)
    got = _check(hip, oracle, cams, depths, normals, images, cases.TWO_CUBED, False, "2x2x2")
    assert got["brick_candidate"].shape == (1, 1, 1) and got["stats"]["tested_bricks"] == 1
    assert len(got["xyz"]) == 1


def test_box_in_free_space(hip, oracle):
    cams, depths, normals, images = cases.inputs(2)
    got = _check(hip, oracle, cams, depths, normals, images, cases.FREE, True, "free-space")
    assert got["stats"] == {"bricks": 4, "seed_bricks": 0, "allocated_bricks": 0,
                            "state_bytes": 0, "tested_bricks": 0}
    assert not got["brick_candidate"].any() and got["xyz"].shape == (0, 3)


def test_box_half_outside_every_frustum(hip, oracle):
    cams, depths, normals, images = cases.inputs(5)
    got = _check(hip, oracle, cams, depths, normals, images, cases.HALF_OUTSIDE, True,
                 "half-outside")
    assert len(got["faces"]) > 100
    assert got["stats"]["tested_bricks"] < got["stats"]["bricks"]


@pytest.mark.parametrize("box", [cases.AROUND_CAMERA, cases.STRADDLE],
                         ids=["around", "across-z0"])
def test_box_around_a_camera_centre(hip, oracle, box):
    cams, depths, normals, images = cases.inputs(5, channels=1)
    got = _check(hip, oracle, cams, depths, normals, images, box, True, "camera-inside")
    assert len(got["faces"]) > 0
    assert got["stats"]["tested_bricks"] < got["stats"]["bricks"]


def test_a_side_of_4096(hip, oracle):
    cams, depths, normals, images = cases.inputs(2)
    got = _check(hip, oracle, cams, depths, normals, images, cases.BAR, True, "4096")
    assert len(got["faces"]) > 100
    assert 5 * got["stats"]["tested_bricks"] <= got["stats"]["bricks"]


@pytest.mark.parametrize("size", [(5, 3), (1, 1)], ids=["5x3", "1x1"])
def test_a_tiny_view(hip, oracle, size):
    """the last of three views has 5 x 3 pixels or one: its pyramid has three
    levels or none"""
    cams, depths, normals, images = cases.inputs(3, last_size=size)
    assert depths[2].shape == size[::-1] and (depths[2] != 0).any()
    got = _check(hip, oracle, cams, depths, normals, images, cases.DEEP, True, "tiny-%dx%d" % size)
    assert len(got["faces"]) > 100
    # and on its own: every voxel in the band of its few pixels
    one = _check(hip, oracle, cams[2:], depths[2:], normals[2:], images[2:], cases.DEEP, False,
                 "only-%dx%d" % size)
    assert one["stats"]["seed_bricks"] > 0


def test_more_than_2_to_the_32_voxels(hip):
    """the 4096 x 4096 x 264 case of tests/test_gpu_tsdf_sparse.py with the
    cull: the same mesh from field_window, and the exact seed test on less
    than a hundredth of the 17 million bricks (DESIGN.md section 9.10 has the
    restatement's count)"""
    origin, voxel, dims = cases.HUGE
    cams, depths, normals, images = cases.huge_inputs()
    got = hip.fuse_tsdf(cams, depths, normals, images, origin, voxel, dims, cut=True,
                        sparse=True, brick_state=True, cull=True, brick_candidate=True)
    want = tsdf_sparse_ref.fuse(cams, depths, images, origin, voxel, dims,
                                window=cases.HUGE_WINDOW)
    st = got["stats"]
    print("TSDF-CULL huge", st)
    _equal(got, want, ("brick_state",) + MESH_KEYS + ("cells",), "huge")
    assert {k: st[k] for k in SPARSE_STATS} == want["stats"]
    assert len(got["faces"]) > 100 and got["cells"].min() < 1 << 32 < got["cells"].max()
    assert st["tested_bricks"] == int(got["brick_candidate"].sum(dtype=np.int64))
    assert np.all((got["brick_state"] == 2) <= (got["brick_candidate"] != 0))
    assert 100 * st["tested_bricks"] <= st["bricks"]
    # the restatement on the slabs of bricks around the window
    lo, hi = cases.HUGE_WINDOW
    slabs = (lo[2] // 4 - 2, hi[2] // 4)
    cand = tsdf_cull_ref.candidates(cams, depths, origin, voxel, dims, bz_range=slabs)
    assert np.array_equal(got["brick_candidate"][slabs[0]:slabs[1]], cand)


@pytest.mark.parametrize("cut", [False, True], ids=["uncut", "cut"])
@pytest.mark.parametrize("w,h", [(97, 63), (80, 71), (5, 3), (1, 1)])
def test_depth_pyramid_is_the_restatements(hip, oracle, w, h, cut):
    """(the cut leaves nothing of a 5 x 3 or 1 x 1 view among larger ones: an
    all-invalid pyramid; uncut they have valid pixels)"""
    cams, depths, normals, images = cases.inputs(3, last_size=(w, h))
    maps = _cut_maps(oracle, cams, depths, normals, cut)
    for view in (2, 0):
        vw, vh = (w, h) if view == 2 else (97, 63)
        want = tsdf_cull_ref.view_pyramids(cams[view:view + 1], maps[view:view + 1])[0][1][1:]
        got = hip.tsdf_depth_pyramid(cams, depths, normals, view, cut=cut)
        levels = int(np.ceil(np.log2(max(vw, vh)))) if max(vw, vh) > 1 else 0
        assert len(got) == len(want) == levels
        for l, ((lo, hi), (wlo, whi)) in enumerate(zip(got, want)):
            assert lo.dtype == hi.dtype == np.float32 and lo.shape == wlo.shape, l
            assert np.array_equal(lo, wlo) and np.array_equal(hi, whi), (view, l)
        if got:
            assert got[-1][0].shape == (1, 1)
            if not cut or view == 0:
                valid = maps[view][maps[view] != 0]
                assert np.isfinite(got[-1][0][0, 0]) and got[-1][0][0, 0] < got[-1][1][0, 0] \
                    or len(valid) < 2


def test_cull_false_is_the_old_entry_with_the_new_stats(hip):
    cams, depths, normals, images = cases.inputs(3)
    origin, voxel, dims = cases.DEEP
    args = (cams, depths, normals, images, origin, voxel, dims)
    old = hip.fuse_tsdf(*args, sparse=True, brick_state=True)
    new = hip.fuse_tsdf(*args, sparse=True, brick_state=True, cull=False, brick_candidate=True)
    _equal(new, old, ("brick_state",) + MESH_KEYS + ("cells",), "cull-off")
    assert new["stats"] == dict(old["stats"], tested_bricks=old["stats"]["bricks"])
    assert new["brick_candidate"].all()


# ------------------------------------------------------------------- the budget
def test_budget(hip):
    from smvs_amd._capi import SmvsError
    cams, depths, normals, images = cases.inputs(3)
    origin, voxel, dims = cases.DEEP
    args = (cams, depths, normals, images, origin, voxel, dims)
    full = hip.fuse_tsdf(*args, sparse=True, cull=True, brick_candidate=True)
    need = full["stats"]["allocated_bricks"]
    assert need > 1
    with pytest.raises(SmvsError) as e:
        hip.fuse_tsdf(*args, sparse=True, cull=True, brick_candidate=True, max_bricks=need - 1)
    assert e.value.status == -4 and str(need) in str(e.value)
    assert e.value.stats == full["stats"] and 0 < e.value.stats["tested_bricks"]
    assert np.array_equal(e.value.brick_candidate, full["brick_candidate"])
    exact = hip.fuse_tsdf(*args, sparse=True, cull=True, max_bricks=need)
    _equal(exact, full, MESH_KEYS + ("cells",), "budget")


def test_budget_leaves_no_handle(hip):
    """the C entry itself: SMVS_ERR_NOMEM, stats and brick_candidate filled, the
    handle NULL"""
    import ctypes as C
    from smvs_amd import _capi
    from smvs_amd.device import _tsdf_views, _tsdf_options
    cams, depths, normals, images = cases.inputs(2)
    lib = _capi.load()
    arr, _keep = _tsdf_views(cams, depths, normals, images)
    origin, voxel, dims = cases.SMALL
    opt = _tsdf_options(origin, voxel, dims, 0.0, True)
    sopt = _capi.TsdfSparseOpts(1, 1)
    stats = _capi.TsdfSparseOptsStats()
    cand = np.full(5 * 4 * 6, 7, np.uint8)
    handle = C.c_void_p(1)
    nv, nf = C.c_int64(-7), C.c_int64(-7)
    rc = lib.smvs_tsdf_fuse_sparse_opts(0, arr, 2, C.byref(opt), C.byref(sopt), None,
                                        cand.ctypes.data_as(C.POINTER(C.c_uint8)), None, None,
                                        C.byref(stats), C.byref(handle), C.byref(nv),
                                        C.byref(nf))
    assert rc == -4 and handle.value is None
    assert stats.bricks == 5 * 4 * 6 and 1 < stats.seed_bricks < stats.allocated_bricks
    assert set(np.unique(cand)) <= {0, 1}
    assert stats.seed_bricks <= stats.tested_bricks == int(cand.sum()) <= stats.bricks


# -------------------------------------------------------------- the scene entry
def test_scene_fused_sparse_cull(hip, tmp_path):
    """host.generate_fused(scene, sparse=True, cull=True) writes the bytes of
    cull=False"""
    from smvs_amd import synth, host, mve_scene
    inputs = synth.pipeline_inputs("sphere", 192, 128, 2, flen=1.2)
    d = str(tmp_path)
    mve_scene.write_scene(d, inputs)
    done, _, _ = host.reconstruct_scene(d, view_ids=[0, 1, 2], num_neighbors=2,
                                        min_neighbors=1, output_scale=2, input_scale=0)
    assert sorted(done) == [0, 1, 2]
    lo, hi = np.float32((-1.0, -0.8, 2.8)), np.float32((1.0, 0.8, 4.3))
    kw = dict(voxel_size=np.float32(0.05), aabb=(lo, hi), input_scale=0, sparse=True)
    path, nv, nf = host.generate_fused(d, **kw)
    with open(path, "rb") as f:
        plain = f.read()
    os.remove(path)
    path2, nv2, nf2 = host.generate_fused(d, cull=True, **kw)
    with open(path2, "rb") as f:
        culled = f.read()
    assert path2 == path and (nv2, nf2) == (nv, nf) and nf > 100
    assert culled == plain
