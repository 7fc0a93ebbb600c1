"""smvs_tsdf_sparse_volume on the device: the persistent brick-sparse volume
fused batch by batch against the one-shot sparse entry on the device
(fuse_tsdf(sparse=True)), its restatement (tests/tsdf_sparse_ref.py) and the
restatement with explicit state (tests/tsdf_sparse_volume_ref.py).  Everything
is compared by array_equal, the NaN positions of the field included, and the
checkpoint byte for byte.  The views and their order are
tests/test_tsdf_sparse_volume_cpu.py's, which shows that growth decides on them."""
import numpy as np
import pytest

import tsdf_sparse_ref  # tests/tsdf_sparse_ref.py
import tsdf_sparse_volume_ref as ref  # tests/tsdf_sparse_volume_ref.py
from test_gpu_tsdf_sparse import DEEP, HUGE, SMALL, _cut_maps, _inputs
from test_tsdf_sparse_volume_cpu import (ALL_KEYS, MESH_KEYS, PARTITIONS, reordered, same,
                                         same_checkpoint)
from test_tsdf_volume_cpu import batches_of

pytestmark = pytest.mark.gpu

OUT_KEYS = ALL_KEYS + ("tsdf",)
ONE_SHOT_STATS = ("bricks", "seed_bricks", "allocated_bricks")


@pytest.fixture(scope="module")
def hip():
    import smvs_amd
    if smvs_amd.device_count() < 1:
        pytest.fail("no HIP device")
    return smvs_amd


@pytest.fixture(scope="module")
def views():
    return reordered(_inputs(5, 97, 63, 3))     # cams, depths, normals, images


def prepared(views, maps=None):
    """(cams, maps, images): what the restatements take"""
    cams, depths, _, images = views
    return cams, depths if maps is None else maps, images


@pytest.fixture(scope="module")
def one_shot(hip, views):
    """the cut off on DEEP: the device's one-shot and the restatement's, which agree"""
    out = {}
    for mw in (1, 2):
        out[mw] = hip.fuse_tsdf(*views, *DEEP, cut=False, volume=True, sparse=True,
                                brick_state=True, min_weight=mw)
        same(out[mw], tsdf_sparse_ref.fuse(*prepared(views), *DEEP, min_weight=mw), OUT_KEYS)
    return out


def volume(hip, box, batches, marks_first=True, cut=False, cull=False, grow=None, **kw):
    """a volume with the batches (cams, depths, normals, images) marked (with
    marks_first) and integrated (grow: off after marks, else on)"""
    vol = hip.SparseTsdfVolume(*box, **kw)
    if marks_first:
        for cams, depths, normals, _ in batches:
            vol.mark(cams, depths, normals, cut=cut, cull=cull)
    if grow is None:
        grow = not marks_first
    for batch in batches:
        vol.integrate(*batch, cut=cut, grow=grow, cull=cull)
    return vol


def same_as_one_shot(got, want, keys=OUT_KEYS):
    same(got, want, keys)
    assert {k: got["stats"][k] for k in ONE_SHOT_STATS} \
        == {k: want["stats"][k] for k in ONE_SHOT_STATS}
    assert got["stats"]["late_bricks"] == 0 and got["stats"]["pending_bricks"] == 0


def same_as_restated(vol, state, min_weight=0):
    got = vol.extract(min_weight=min_weight, volume=True, brick_state=True)
    want = ref.extract(state, min_weight)
    same(got, want, OUT_KEYS)
    assert got["stats"] == want["stats"] == vol.stats()
    assert set(got) == set(want)
    same_checkpoint(vol.state(), ref.checkpoint(state))
    return got


# ------------------------------------------------------------ 1. marks first
@pytest.mark.parametrize("partition", PARTITIONS, ids=str)
def test_marks_first_is_the_one_shot(hip, views, one_shot, partition):
    with volume(hip, DEEP, batches_of(partition, *views)) as vol:
        assert vol.n_views == 5
        before = vol.state()
        got = vol.extract(volume=True, brick_state=True)
        second = vol.extract(min_weight=2, volume=True, brick_state=True)
        same_checkpoint(vol.state(), before)
        state = ref.fuse_batches(batches_of(partition, *prepared(views)), *DEEP)
        same_as_restated(vol, state)
    same_as_one_shot(got, one_shot[1])
    same_as_one_shot(second, one_shot[2])
    assert np.array_equal(np.isnan(got["tsdf"]), np.isnan(one_shot[1]["tsdf"]))
    assert got["stats"]["allocated_bricks"] == 290 and got["stats"]["state_bytes"] == 290 * 6144
    assert len(got["faces"]) > 100 and got["faces"].max() < len(got["xyz"])
    assert np.isnan(second["tsdf"]).sum() > np.isnan(got["tsdf"]).sum()


def test_marks_first_on_sides_that_are_no_multiple_of_a_brick(hip, views):
    want = hip.fuse_tsdf(*views, *SMALL, cut=False, volume=True, sparse=True, brick_state=True)
    with volume(hip, SMALL, batches_of((2, 3), *views)) as vol:
        same_as_one_shot(vol.extract(volume=True, brick_state=True), want)
        same_as_restated(vol, ref.fuse_batches(batches_of((2, 3), *prepared(views)), *SMALL))


def test_normals_and_images_are_not_needed_where_they_are_not_read(hip, views, one_shot):
    cams, depths, _, images = views
    with hip.SparseTsdfVolume(*DEEP) as vol:
        vol.mark(cams, depths, None, cut=False)
        vol.integrate(cams[:2], depths[:2], None, images[:2], cut=False, grow=False)
        vol.integrate(cams[2:], depths[2:], None, images[2:], cut=False, grow=False)
        got = vol.extract()
    assert set(got) == set(MESH_KEYS) | {"cells", "stats"}
    same(got, one_shot[1], MESH_KEYS + ("cells",))


# ----------------------------------------------------------- 2. growth only
@pytest.mark.parametrize("partition,late", [((4, 1), 48), ((2, 3), 52)], ids=str)
def test_growth_only_is_the_restatement(hip, views, one_shot, partition, late):
    state = ref.fuse_batches(batches_of(partition, *prepared(views)), *DEEP, marks_first=False)
    with volume(hip, DEEP, batches_of(partition, *views), marks_first=False) as vol:
        got = same_as_restated(vol, state)
        birth = vol.state()["birth"]
    assert got["stats"]["late_bricks"] == late == int((birth > 0).sum())
    assert set(np.unique(birth)) == {0, partition[0]}
    same(got, one_shot[1], ("brick_state",))
    if partition == (4, 1):
        assert len(got["xyz"]) != len(one_shot[1]["xyz"])
    else:
        same(got, one_shot[1], MESH_KEYS + ("cells",))


# ----------------------------------------------------------------- 3. mixed
def test_marks_up_front_and_a_view_that_arrives_later(hip, views):
    first, second = batches_of((4, 1), *views)
    rfirst, rsecond = batches_of((4, 1), *prepared(views))
    state = ref.integrate(ref.mark(ref.create(*DEEP), *rfirst[:2]), *rfirst, grow=False)
    with hip.SparseTsdfVolume(*DEEP) as vol:
        vol.mark(*first[:3], cut=False)
        vol.integrate(*first, cut=False, grow=False)
        same_as_restated(vol, state)
        assert vol.stats()["late_bricks"] == 0
        vol.integrate(*second, cut=False, grow=True)
        got = same_as_restated(vol, ref.integrate(state, *rsecond, grow=True))
    assert got["stats"]["late_bricks"] == 48 and got["stats"]["n_views"] == 5


# --------------------------------------------------------------- 4. re-slot
def test_a_re_slot_keeps_the_sums_at_their_new_slots(hip, views):
    first, second = batches_of((4, 1), *views)
    with hip.SparseTsdfVolume(*DEEP) as vol:
        vol.integrate(*first, cut=False, grow=True)
        a = vol.state()
        vol.mark(*second[:3], cut=False)
        pending = vol.stats()["pending_bricks"]
        assert pending == 48 and vol.stats()["allocated_bricks"] == len(a["list"])
        same_checkpoint({**vol.state(), "brick_state": a["brick_state"]}, a)
        # a view without a valid pixel: the table changes, no sum does
        blind = [np.zeros_like(second[1][0])]
        vol.integrate(second[0], blind, second[2], second[3], cut=False, grow=False)
        b = vol.state()
    assert len(b["list"]) == len(a["list"]) + pending and b["n_views"] == 5
    at = np.searchsorted(b["list"], a["list"])
    assert np.array_equal(b["list"][at], a["list"]) and np.any(at != np.arange(len(at)))
    for k in ("S", "W", "rgbc", "birth"):
        assert b[k][at].tobytes() == a[k].tobytes(), k
    new = np.setdiff1d(np.arange(len(b["list"])), at)
    assert not b["W"][new].any() and not b["S"][new].any() and not b["rgbc"][new].any()
    assert np.all(b["birth"][new] == 4)


# -------------------------------------------------------- 5. superset marks
def test_marks_of_views_never_integrated_do_not_change_the_mesh(hip, views):
    four = tuple(x[:4] for x in views)
    want = hip.fuse_tsdf(*four, *DEEP, cut=False, sparse=True, brick_state=True)
    with hip.SparseTsdfVolume(*DEEP) as vol:
        vol.mark(*views[:3], cut=False)
        vol.integrate(*four, cut=False, grow=False)
        got = vol.extract(brick_state=True)
    assert got["stats"]["allocated_bricks"] == 290 > want["stats"]["allocated_bricks"]
    same(got, want, MESH_KEYS + ("cells",))
    assert not np.array_equal(got["brick_state"], want["brick_state"])


# ---------------------------------------------------------------- 6. cut on
def test_one_batch_with_the_cut_is_the_one_shot(hip, views):
    want = hip.fuse_tsdf(*views, *DEEP, cut=True, volume=True, sparse=True, brick_state=True)
    for marks_first in (True, False):
        with volume(hip, DEEP, [views], marks_first=marks_first, cut=True) as vol:
            same_as_one_shot(vol.extract(volume=True, brick_state=True), want)


@pytest.mark.parametrize("partition", [(2, 3), (1, 4)], ids=str)
def test_the_cut_acts_within_a_batch(hip, oracle, views, partition):
    cams, depths, normals, images = views
    batches = batches_of(partition, *views)
    # the oracle's cut maps per batch (a batch of one view is not cut), concatenated
    dms = []
    for c, d, n, _ in batches:
        dms += list(_cut_maps(oracle, c, d, n, True))
    assert any(not np.array_equal(a, b) for a, b in zip(dms, depths))
    want = tsdf_sparse_ref.fuse(cams, dms, images, *DEEP)
    with volume(hip, DEEP, batches, cut=True) as vol:
        got = same_as_restated(vol, ref.fuse_batches(batches_of(partition, cams, dms, images),
                                                     *DEEP))
    same_as_one_shot(got, want)
    assert len(got["faces"]) > 100


# ------------------------------------------------------------------ 7. cull
@pytest.mark.parametrize("marks_first", [True, False], ids=["marks", "growth"])
def test_the_cull_decides_nothing(hip, views, marks_first):
    batches = batches_of((2, 3), *views)
    with volume(hip, DEEP, batches, marks_first=marks_first, cull=False) as a, \
            volume(hip, DEEP, batches, marks_first=marks_first, cull=True) as b:
        same_checkpoint(b.state(), a.state())
        assert a.stats() == b.stats()
        same(b.extract(volume=True, brick_state=True), a.extract(volume=True, brick_state=True),
             OUT_KEYS)


# ------------------------------------------- 8.-10. checkpoint, reset, volumes
def test_checkpoint_continues_to_the_same_bits(hip, views, one_shot):
    first, second = batches_of((2, 3), *views)
    with hip.SparseTsdfVolume(*DEEP) as vol:
        vol.mark(*views[:3], cut=False)
        vol.integrate(*first, cut=False, grow=False)
        saved = vol.state()
    assert saved["n_views"] == 2 and len(saved["list"]) == 290
    with hip.SparseTsdfVolume(*DEEP) as vol:
        vol.load_state(**saved)
        assert vol.n_views == 2
        same_checkpoint(vol.state(), saved)
        vol.integrate(*second, cut=False, grow=False)
        same_as_one_shot(vol.extract(volume=True, brick_state=True), one_shot[1])
    # a growth-only state, with its births
    with volume(hip, DEEP, [first], marks_first=False) as vol:
        saved = vol.state()
    with hip.SparseTsdfVolume(*DEEP) as vol:
        vol.load_state(**saved)
        vol.integrate(*second, cut=False, grow=True)
        resumed = vol.state()
        assert vol.stats()["late_bricks"] == 52
    with volume(hip, DEEP, [first, second], marks_first=False) as vol:
        same_checkpoint(resumed, vol.state())
    with pytest.raises(ValueError):
        with hip.SparseTsdfVolume(*SMALL) as vol:
            vol.load_state(**saved)


def test_reset(hip, views, one_shot):
    with volume(hip, DEEP, batches_of((4, 1), *views), marks_first=False) as vol:
        assert vol.stats()["late_bricks"] == 48
        vol.reset()
        assert vol.stats() == {"bricks": 1064, "seed_bricks": 0, "allocated_bricks": 0,
                               "pending_bricks": 0, "late_bricks": 0, "state_bytes": 0,
                               "n_views": 0}
        empty = vol.extract(volume=True, brick_state=True)
        assert np.isnan(empty["tsdf"]).all() and not empty["brick_state"].any()
        assert empty["xyz"].shape == (0, 3) and empty["faces"].shape == (0, 3)
        assert vol.state()["S"].shape == (0, 256)
        for batch in batches_of((3, 2), *views):
            vol.mark(*batch[:3], cut=False)
        for batch in batches_of((3, 2), *views):
            vol.integrate(*batch, cut=False, grow=False)
        same_as_one_shot(vol.extract(volume=True, brick_state=True), one_shot[1])


def test_two_volumes_side_by_side(hip, views, one_shot):
    want_small = hip.fuse_tsdf(*views, *SMALL, cut=False, volume=True, sparse=True,
                               brick_state=True)
    a = hip.SparseTsdfVolume(*DEEP)
    b = hip.SparseTsdfVolume(*SMALL)
    try:
        first, second = batches_of((2, 3), *views)
        for batch in (first, second):
            a.mark(*batch[:3], cut=False)
            b.mark(*batch[:3], cut=False)
        a.integrate(*first, cut=False, grow=False)
        b.integrate(*first, cut=False, grow=False)
        b.integrate(*second, cut=False, grow=False)
        same_as_one_shot(b.extract(volume=True, brick_state=True), want_small)
        a.integrate(*second, cut=False, grow=False)
        same_as_one_shot(a.extract(volume=True, brick_state=True), one_shot[1])
        same_as_one_shot(b.extract(volume=True, brick_state=True), want_small)
    finally:
        a.close()
        b.close()
    with pytest.raises(ValueError, match="closed"):
        a.extract()


# ------------------------------------------------ 11. a batch that looks away
def test_a_batch_that_contributes_nothing(hip, views, one_shot):
    cams, depths, normals, images = views
    blind = [np.zeros_like(d) for d in depths[:2]]      # no valid pixel: D == 0 everywhere
    with volume(hip, DEEP, batches_of((2, 3), *views)) as vol:
        before = vol.state()
        vol.mark(cams[:2], blind, normals[:2], cut=False)
        vol.integrate(cams[:2], blind, normals[:2], images[:2], cut=False, grow=True)
        after = vol.state()
        assert after.pop("n_views") == 7 and before.pop("n_views") == 5
        same_checkpoint({**after, "n_views": 0}, {**before, "n_views": 0})
        got = vol.extract(volume=True, brick_state=True)
    # the sums are the 5 views', the confidences follow the 7
    same(got, one_shot[1], [k for k in OUT_KEYS if k != "confidence"])
    assert (got["confidence"] < one_shot[1]["confidence"]).all()


# --------------------------------------- 12., 13. other sizes, other channels
def test_a_view_of_another_size_and_an_explicit_truncation(hip):
    views = reordered(_inputs(5, 97, 63, 3, last_size=(80, 71)))
    assert views[1][3].shape == (71, 80) != views[1][0].shape
    want = hip.fuse_tsdf(*views, *DEEP, trunc=0.1, cut=False, volume=True, sparse=True,
                         brick_state=True)
    with volume(hip, DEEP, batches_of((2, 3), *views), trunc=0.1) as vol:
        same_as_one_shot(vol.extract(volume=True, brick_state=True), want)
        same_as_restated(vol, ref.fuse_batches(batches_of((2, 3), *prepared(views)), *DEEP,
                                               trunc=0.1))
    assert len(want["faces"]) > 100


def test_single_channel_images(hip):
    views = reordered(_inputs(5, 97, 63, 1))
    assert views[3][0].ndim == 2
    want = hip.fuse_tsdf(*views, *DEEP, cut=False, volume=True, sparse=True, brick_state=True)
    with volume(hip, DEEP, batches_of((4, 1), *views)) as vol:
        got = vol.extract(volume=True, brick_state=True)
    same_as_one_shot(got, want)
    assert np.all(got["rgb"][:, 0] == got["rgb"][:, 1]) and got["rgb"].any()
    with volume(hip, DEEP, batches_of((4, 1), *views), marks_first=False) as vol:
        same_as_restated(vol, ref.fuse_batches(batches_of((4, 1), *prepared(views)), *DEEP,
                                               marks_first=False))


# --------------------------------------------------------------- 14. budget
def test_the_budget_is_checked_before_anything_changes(hip, views, one_shot):
    from smvs_amd._capi import SmvsError
    first, second = batches_of((4, 1), *views)
    need = one_shot[1]["stats"]["allocated_bricks"]
    assert need == 290
    with hip.SparseTsdfVolume(*DEEP, max_bricks=need - 1) as vol:
        vol.integrate(*first, cut=False, grow=True)
        before = vol.state()
        stats = vol.stats()
        assert stats["allocated_bricks"] == 242
        for call in (lambda: vol.mark(*second[:3], cut=False),
                     lambda: vol.mark(*second[:3], cut=False, cull=True),
                     lambda: vol.integrate(*second, cut=False, grow=True)):
            with pytest.raises(SmvsError) as e:
                call()
            assert e.value.status == -4 and str(need) in str(e.value)
            assert vol.stats() == stats
            same_checkpoint(vol.state(), before)
        # without growth the view is summed on the bricks there are
        vol.integrate(*second, cut=False, grow=False)
        assert vol.n_views == 5 and vol.stats()["allocated_bricks"] == 242
    # the next call with a larger budget works
    with hip.SparseTsdfVolume(*DEEP, max_bricks=need) as vol:
        vol.load_state(**before)
        vol.integrate(*second, cut=False, grow=True)
        assert vol.stats()["allocated_bricks"] == need
        with volume(hip, DEEP, [first, second], marks_first=False) as free:
            same_checkpoint(vol.state(), free.state())


# ------------------------------------------------------------- 15. refusals
def test_refusals_leave_the_volume_usable(hip, views, one_shot):
    import ctypes as C
    from smvs_amd import _capi
    from smvs_amd._capi import SmvsError
    from smvs_amd.device import _tsdf_views
    first, second = batches_of((2, 3), *views)

    def refused(call):
        with pytest.raises(SmvsError) as e:
            call()
        assert e.value.status == -1

    refused(lambda: hip.SparseTsdfVolume(DEEP[0], 0.0, DEEP[2]))
    refused(lambda: hip.SparseTsdfVolume(DEEP[0], DEEP[1], (37, 1, 23)))
    refused(lambda: hip.SparseTsdfVolume(DEEP[0], DEEP[1], (37, 4097, 23)))
    refused(lambda: hip.SparseTsdfVolume((0.0, float("nan"), 0.0), DEEP[1], DEEP[2]))
    refused(lambda: hip.SparseTsdfVolume(*DEEP, trunc=float("inf")))
    refused(lambda: hip.SparseTsdfVolume(*DEEP, max_bricks=(1 << 23) + 1))
    lib = _capi.load()
    with hip.SparseTsdfVolume(*DEEP) as vol:
        vol.mark(*views[:3], cut=False)
        vol.integrate(*first, cut=False, grow=False)
        before = vol.state()
        stats = vol.stats()
        # what check_views refuses
        refused(lambda: vol.mark([], [], [], cut=False))
        refused(lambda: vol.integrate([], [], [], [], cut=False))
        refused(lambda: vol.mark(*second[:2], None, cut=True))
        refused(lambda: vol.integrate(*second[:2], None, second[3], cut=True))
        for change in ("channels", "image", "depth"):
            arr, _keep = _tsdf_views(*second)
            if change == "channels":
                arr[1].channels = 5
            else:
                setattr(arr[1], change, None)
            assert lib.smvs_tsdf_sparse_volume_integrate(vol._handle, arr, 3, 0, 1, 0) == -1, change
            # mark reads no image
            assert lib.smvs_tsdf_sparse_volume_mark(vol._handle, arr, 3, 0, 0) \
                == (-1 if change == "depth" else 0), change
        arr, _keep = _tsdf_views(*second)
        assert lib.smvs_tsdf_sparse_volume_integrate(vol._handle, arr, 4097, 0, 1, 0) == -1
        assert lib.smvs_tsdf_sparse_volume_mark(vol._handle, arr, 4097, 0, 0) == -1
        # the checkpoint's checks
        bad = dict(before)
        refused(lambda: vol.load_state(**{**bad, "n_views": -1}))
        refused(lambda: vol.load_state(**{**bad, "n_views": (1 << 24) + 1}))
        refused(lambda: vol.load_state(**{**bad, "birth": before["birth"] + 3}))   # above n_views
        swapped = before["list"].copy()
        swapped[[3, 4]] = swapped[[4, 3]]
        refused(lambda: vol.load_state(**{**bad, "list": swapped}))
        outside = before["list"].copy()
        outside[-1] = 1064
        refused(lambda: vol.load_state(**{**bad, "list": outside}))
        refused(lambda: vol.load_state(**{**bad,
                                          "brick_state": np.zeros_like(before["brick_state"])}))
        refused(lambda: vol.load_state(**{**bad,
                                          "brick_state": np.full_like(before["brick_state"], 3)}))
        assert lib.smvs_tsdf_sparse_volume_upload(vol._handle, None, None, None, C.c_int64(0),
                                                  None, None, None, C.c_int64(2)) == -1
        # no handle pointer
        assert lib.smvs_tsdf_sparse_volume_extract(vol._handle, 0, None, None, None, None, None,
                                                   None) == -1
        assert vol.stats() == stats
        same_checkpoint(vol.state(), before)
        # the view count: 2^24 in all
        vol.load_state(**{**before, "n_views": (1 << 24) - 2})
        refused(lambda: vol.integrate(*second, cut=False, grow=False))
        assert vol.n_views == (1 << 24) - 2
        vol.load_state(**before)
        same_checkpoint(vol.state(), before)
        # and the volume goes on as if nothing had been asked
        vol.integrate(*second, cut=False, grow=False)
        same_as_one_shot(vol.extract(volume=True, brick_state=True), one_shot[1])
    with hip.SparseTsdfVolume(*HUGE) as vol:
        # tsdf / weight only up to 2^27 voxels (refused before anything is allocated for them)
        mesh = C.c_void_p(1)
        one = (C.c_float * 1)()
        assert lib.smvs_tsdf_sparse_volume_extract(vol._handle, 0, None, one, None, C.byref(mesh),
                                                   None, None) == -1
        assert mesh.value is None


# ----------------------------------------------------------- 16. a large grid
def test_more_than_2_to_the_32_voxels_in_two_batches(hip):
    """4096 x 4096 x 264 voxels and two narrow 32 x 24 views, one per batch,
    marked with the cull in front: mesh, cells (above 2^32 too) and stats are
    the one-shot sparse entry's."""
    from smvs_amd import synth
    origin, voxel, dims = HUGE
    cams = [synth.Camera(np.eye(3), np.zeros(3), 8.0, 32, 24),
            synth.Camera(np.eye(3), np.array([0.02, -0.01, 0.0]), 8.0, 32, 24)]
    depths, normals = synth.depth_and_normal_maps(synth.SphereScene(), cams)
    rng = np.random.default_rng(3)
    images = [rng.integers(0, 256, (24, 32, 3)).astype(np.uint8) for _ in cams]
    depths[0][5, 7] = 0.0
    want = hip.fuse_tsdf(cams, depths, normals, images, origin, voxel, dims, cut=False,
                         sparse=True, brick_state=True, cull=True)
    alone = hip.fuse_tsdf(cams[:1], depths[:1], normals[:1], images[:1], origin, voxel, dims,
                          cut=False, sparse=True, cull=True)
    assert want["stats"]["allocated_bricks"] > alone["stats"]["allocated_bricks"]
    batches = batches_of((1, 1), cams, depths, normals, images)
    with volume(hip, HUGE, batches, cull=True) as vol:
        got = vol.extract(brick_state=True)
    same(got, want, ("brick_state",) + MESH_KEYS + ("cells",))
    assert {k: got["stats"][k] for k in ONE_SHOT_STATS} \
        == {k: want["stats"][k] for k in ONE_SHOT_STATS}
    assert got["stats"]["late_bricks"] == 0 and got["stats"]["n_views"] == 2
    assert len(got["faces"]) > 100
    assert got["cells"].min() < 1 << 32 < got["cells"].max()


# -------------------------------------------------------- 17. the scene entry
@pytest.fixture(scope="module")
def scene(hip, tmp_path_factory):
    """a scene written and reconstructed as tests/test_gpu_tsdf_volume.py's"""
    from smvs_amd import synth, host, mve_scene
    inputs = synth.pipeline_inputs("sphere", 192, 128, 2, flen=1.2)
    d = str(tmp_path_factory.mktemp("scene"))
    mve_scene.write_scene(d, inputs)
    done, _, _ = host.reconstruct_scene(d, view_ids=[0, 1, 2], num_neighbors=2,
                                        min_neighbors=1, output_scale=2, input_scale=0)
    assert sorted(done) == [0, 1, 2]
    return d


AABB = (np.float32((-1.0, -0.8, 2.8)), np.float32((1.0, 0.8, 4.3)))


@pytest.mark.parametrize("label,options", [
    ("bounds", dict(resolution=64)),
    ("aabb-cull", dict(voxel_size=np.float32(0.05), aabb=AABB, cull=True)),
    ("clean", dict(resolution=64, clean=dict(percentile=10, component_size=50)))])
def test_scene_sparse_batched_is_the_one_shot_file(hip, scene, label, options):
    import os
    from smvs_amd import host
    results = {}
    for n in (0, 2, 1):
        out = host.generate_fused(scene, input_scale=0, cut=False, sparse=True,
                                  sparse_batch_views=n, **options)
        with open(out[0], "rb") as f:
            results[n] = (os.path.basename(out[0]),) + tuple(out[1:]) + (f.read(),)
        os.remove(out[0])
    name, nv, nf = results[0][:3]
    assert name == ("smvs-clean-B0.ply" if label == "clean" else "smvs-fused-B0.ply")
    assert nf > 100 and len(results[0][-1]) > 1000
    assert results[2] == results[0] and results[1] == results[0]


def test_scene_sparse_batches_belong_to_the_sparse_volume(hip, scene):
    from smvs_amd import host
    from smvs_amd._capi import SmvsError
    with pytest.raises(ValueError, match="sparse_batch_views belongs to sparse"):
        host.generate_fused(scene, resolution=64, input_scale=0, cut=False, sparse_batch_views=2)
    with pytest.raises(SmvsError, match="sparse_batch_views"):
        host.generate_fused(scene, resolution=64, input_scale=0, cut=False, sparse=True,
                            sparse_batch_views=-1)
    with pytest.raises(SmvsError, match="batch_views belongs to the dense volume"):
        host.generate_fused(scene, resolution=64, input_scale=0, cut=False, sparse=True,
                            batch_views=2, sparse_batch_views=2)
    # the budget reaches the scene entry
    with pytest.raises(SmvsError, match="max_bricks"):
        host.generate_fused(scene, resolution=64, input_scale=0, cut=False, sparse=True,
                            sparse_batch_views=2, max_bricks=1)
    # the cut, when on, acts within a batch: one batch of all views is the one-shot
    a = host.generate_fused(scene, resolution=64, input_scale=0, cut=True, sparse=True,
                            sparse_batch_views=3)
    with open(a[0], "rb") as f:
        batched = f.read()
    b = host.generate_fused(scene, resolution=64, input_scale=0, cut=True, sparse=True)
    with open(b[0], "rb") as f:
        assert f.read() == batched and a == b


# ------------------------------- 18. the six C entries state the same request
def test_a_wider_entry_with_the_narrower_options_unset_is_the_narrower_entry(hip, scene):
    """The six smvs_host_generate_fused* entries through ctypes, with records
    that state the same request: file name, counts, the clean's stats and the
    file's bytes are equal within the dense group, the sparse group (the cull
    changes no byte) and the clean group, dense and sparse."""
    import ctypes as C
    import os
    from smvs_amd import _capi, host
    lib = host.load()
    records = dict(_fused=host.FusedSettings, _fused_sparse=host.FusedSparseSettings,
                   _fused_sparse_cull=host.FusedSparseCullSettings,
                   _fused_clean=host.FusedCleanSettings, _fused_batched=host.FusedBatchedSettings,
                   _fused_sparse_batched=host.FusedSparseBatchedSettings)

    def call(entry, cull=0, sparse=0, clean=0):
        # (voxel_size, resolution, trunc, min_weight, max_bricks, cull, sparse, threshold,
        # percentile, component_size, keep_unreferenced, clean, batch_views, sparse_batch_views)
        widest = (0.05, 0, 0.0, 0, 0, cull, sparse, 0.0, 10.0 if clean else 0.0,
                  50 if clean else 1000, 0, clean, 0, 0)
        fs = records[entry](*widest[:len(records[entry]._fields_)])
        st = host._point_cloud_settings("undistorted", 0, False, False, AABB, True, False, 0)
        path = C.create_string_buffer(4096)
        nv, nf = C.c_int64(0), C.c_int64(0)
        args = [scene.encode(), C.byref(st), C.byref(fs), None, C.c_int(0), path,
                C.c_int(len(path)), C.byref(nv), C.byref(nf)]
        stats = _capi.MeshCleanStats()
        if entry in ("_fused_clean", "_fused_batched", "_fused_sparse_batched"):
            args.append(C.byref(stats))
        rc = getattr(lib, "smvs_host_generate" + entry)(*args)
        assert rc == 0, (entry, lib.smvs_host_last_error().decode())
        with open(path.value.decode(), "rb") as f:
            data = f.read()
        os.remove(path.value.decode())
        return (os.path.basename(path.value.decode()), nv.value, nf.value, stats.as_dict(), data)

    def all_equal(results, name):
        assert results[0][0] == name and results[0][2] > 100 and len(results[0][4]) > 1000
        for r in results[1:]:
            assert r == results[0]
        return results[0]

    dense = all_equal([call("_fused"), call("_fused_batched"), call("_fused_sparse_batched")],
                      "smvs-fused-B0.ply")
    sparse = all_equal([call("_fused_sparse"), call("_fused_sparse_cull", cull=0),
                        call("_fused_sparse_cull", cull=1), call("_fused_batched", sparse=1),
                        call("_fused_sparse_batched", sparse=1)], "smvs-fused-B0.ply")
    # the same mesh in another order (section 9.9), and no clean has counted
    assert sparse[1:3] == dense[1:3] and sparse[4] != dense[4]
    assert dense[3] == sparse[3] == _capi.MeshCleanStats().as_dict()
    for s in (0, 1):
        cleaned = all_equal([call("_fused_clean", sparse=s, clean=1),
                             call("_fused_batched", sparse=s, clean=1),
                             call("_fused_sparse_batched", sparse=s, clean=1)],
                            "smvs-clean-B0.ply")
        assert cleaned[3]["n_components"] >= 1 and 0 < cleaned[1] <= dense[1]
