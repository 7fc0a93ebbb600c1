"""The persistent brick-sparse fusion volume on the CPU: the numpy restatement
with explicit state (tests/tsdf_sparse_volume_ref.py) against the one-shot
sparse restatement (tests/tsdf_sparse_ref.py) for marks-first, growth-only and
superset-mark sequences; the counts that show that these inputs exercise
growth (a growth test cannot pass with nothing late); and the refusals of the C
ABI, which come before any device call.

The views are the suite's five sphere views in the order [1, 2, 3, 4, 0]: view
0, with its depth step, comes last, after the others have seen free space
where its step puts new seed bricks."""
import ctypes as C

import numpy as np
import pytest

import tsdf_sparse_ref  # tests/tsdf_sparse_ref.py
import tsdf_sparse_volume_ref as ref  # tests/tsdf_sparse_volume_ref.py
from test_gpu_tsdf_sparse import DEEP, SMALL, _inputs
from test_tsdf_volume_cpu import batches_of

ORDER = [1, 2, 3, 4, 0]
PARTITIONS = [(5,), (4, 1), (2, 3), (1, 1, 1, 1, 1)]
MESH_KEYS = ("xyz", "normals", "rgb", "confidence", "faces")
ALL_KEYS = ("brick_state", "weight") + MESH_KEYS + ("cells",)
BOXES = {"37x29x23": SMALL, "61x53x75": DEEP}


def reordered(views):
    """each list of the views in ORDER"""
    return tuple([x[i] for i in ORDER] for x in views)


def same(got, want, keys=ALL_KEYS + ("tsdf",)):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k], equal_nan=(k == "tsdf")), k


def same_checkpoint(got, want):
    assert got["n_views"] == want["n_views"]
    for k in ("brick_state", "list", "birth", "S", "W", "rgbc"):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert got[k].tobytes() == want[k].tobytes(), k


@pytest.fixture(scope="module")
def views():
    cams, depths, _, images = reordered(_inputs(5, 97, 63, 3))
    return cams, depths, images       # the cut is off: the maps are the depth maps


@pytest.fixture(scope="module")
def one_shot(views):
    return {name: tsdf_sparse_ref.fuse(*views, *box) for name, box in BOXES.items()}


@pytest.fixture(scope="module")
def marked_first(views):
    """DEEP, per partition: every batch marked, then every batch integrated"""
    return {p: ref.fuse_batches(batches_of(p, *views), *DEEP) for p in PARTITIONS}


# ---------------------------------------------------------------- marks first
@pytest.mark.parametrize("partition", PARTITIONS, ids=str)
def test_marks_first_is_the_one_shot(views, one_shot, marked_first, partition):
    state = marked_first[partition]
    want = one_shot["61x53x75"]
    got = ref.extract(state)
    same(got, want)
    st = got["stats"]
    assert st["late_bricks"] == 0 and st["pending_bricks"] == 0 and st["n_views"] == 5
    assert {k: st[k] for k in ("bricks", "seed_bricks", "allocated_bricks")} \
        == {k: want["stats"][k] for k in ("bricks", "seed_bricks", "allocated_bricks")}
    assert st["bricks"] == 1064 and st["allocated_bricks"] == 290
    assert st["state_bytes"] == 290 * 6144
    same_checkpoint(ref.checkpoint(state), ref.checkpoint(marked_first[(5,)]))
    # another min_weight from the same state
    same(ref.extract(state, 2), tsdf_sparse_ref.fuse(*views, *DEEP, min_weight=2))


def test_marks_first_on_sides_that_are_no_multiple_of_a_brick(views, one_shot):
    state = ref.fuse_batches(batches_of((2, 3), *views), *SMALL)
    same(ref.extract(state), one_shot["37x29x23"])
    cp = ref.checkpoint(state)
    assert cp["S"].shape == (len(cp["list"]), 256) and cp["rgbc"].shape[1:] == (256, 4)
    assert np.all(np.diff(cp["list"].astype(np.int64)) > 0) and not cp["birth"].any()
    # the lanes of a partial brick that lie outside the grid hold zeros
    last = cp["list"] == cp["list"].max()
    assert (37 % 8, 29 % 8, 23 % 4) == (5, 5, 3)
    lanes = np.arange(256)
    outside = ((lanes & 7) >= 5) | ((lanes >> 3 & 7) >= 5) | ((lanes >> 6) >= 3)
    assert not cp["W"][last][:, outside].any() and cp["W"][last][:, ~outside].any()


# ---------------------------------------------------------------- growth only
GROWTH = {
    # partition: late bricks, voxels where W differs, where F differs, vertices, faces
    (4, 1): (48, 10161, 1277, 2712, 5180),
    (2, 3): (52, 9006, 165, 2587, 4960),
}


@pytest.mark.parametrize("partition", sorted(GROWTH), ids=str)
def test_growth_only_misses_what_the_late_bricks_did_not_see(views, one_shot, marked_first,
                                                             partition):
    late, n_w, n_f, n_vertices, n_faces = GROWTH[partition]
    want = one_shot["61x53x75"]
    assert (len(want["xyz"]), len(want["faces"])) == (2587, 4960)
    state = ref.fuse_batches(batches_of(partition, *views), *DEEP, marks_first=False)
    full = marked_first[partition]
    got = ref.extract(state)
    st = got["stats"]
    # the same bricks in the end, but some of them late
    assert np.array_equal(state["slots"], full["slots"])
    assert np.array_equal(got["brick_state"], want["brick_state"])
    w_differs = int((state["W"] != full["W"]).sum())
    Fa, Fb = got["tsdf"], want["tsdf"]
    f_differs = int((~((Fa == Fb) | (np.isnan(Fa) & np.isnan(Fb)))).sum())
    print("TSDF-SPARSE-VOLUME growth %s: late %d, W differs at %d voxels, F at %d, "
          "%d vertices, %d faces" % (partition, st["late_bricks"], w_differs, f_differs,
                                     len(got["xyz"]), len(got["faces"])))
    assert st["late_bricks"] == late and st["allocated_bricks"] == 290
    assert (w_differs, f_differs) == (n_w, n_f)
    assert (len(got["xyz"]), len(got["faces"])) == (n_vertices, n_faces)
    # late bricks hold the sums of the views from their birth on, the others all
    assert set(np.unique(state["birth"][state["slots"]])) == {0, partition[0]}
    assert np.all(state["W"] <= full["W"])
    early = tsdf_sparse_ref._voxel_mask(state["birth"] == 0, state["W"].shape)
    assert np.array_equal(state["W"][early], full["W"][early])
    assert np.array_equal(state["S"][early], full["S"][early])
    if partition == (4, 1):
        assert not np.array_equal(got["faces"], want["faces"])
    else:
        same(got, want, MESH_KEYS + ("cells",))


def test_mixed_marks_and_growth(views, marked_first):
    """views 1-4 marked up front, view 0 arrives with grow: its new bricks are late"""
    first, second = batches_of((4, 1), *views)
    state = ref.mark(ref.create(*DEEP), *first[:2])
    state = ref.integrate(state, *first, grow=False)
    assert ref.stats(state)["late_bricks"] == 0
    state = ref.integrate(state, *second, grow=True)
    st = ref.stats(state)
    assert st["late_bricks"] == 48 and st["allocated_bricks"] == 290 and st["n_views"] == 5
    grown = ref.fuse_batches([first, second], *DEEP, marks_first=False)
    same_checkpoint(ref.checkpoint(state), ref.checkpoint(grown))


def test_a_re_slot_keeps_the_sums(views):
    first, second = batches_of((4, 1), *views)
    before = ref.integrate(ref.create(*DEEP), *first)
    # view 0 marked, then a view without a valid pixel integrated: the table alone changes
    blind = [np.zeros_like(second[1][0])]
    after = ref.integrate(ref.mark(before, *second[:2]), second[0], blind, second[2], grow=False)
    a, b = ref.checkpoint(before), ref.checkpoint(after)
    assert len(b["list"]) == len(a["list"]) + 48
    at = np.searchsorted(b["list"], a["list"])
    assert np.array_equal(b["list"][at], a["list"]) and np.any(at != np.arange(len(at)))
    for k in ("S", "W", "rgbc", "birth"):
        assert b[k][at].tobytes() == a[k].tobytes(), k
    new = np.setdiff1d(np.arange(len(b["list"])), at)
    assert not b["W"][new].any() and np.all(b["birth"][new] == 4)


# ------------------------------------------------------------- superset marks
def test_marks_of_views_never_integrated_do_not_change_the_mesh(views):
    four = tuple(x[:4] for x in views)
    want = tsdf_sparse_ref.fuse(*four, *DEEP)
    state = ref.mark(ref.create(*DEEP), *views[:2])
    state = ref.integrate(state, *four, grow=False)
    got = ref.extract(state)
    assert got["stats"]["allocated_bricks"] == 290 > want["stats"]["allocated_bricks"]
    same(got, want, MESH_KEYS + ("cells",))
    assert not np.array_equal(got["brick_state"], want["brick_state"])


@pytest.mark.parametrize("name", sorted(BOXES))
def test_every_brick_allocated_is_still_the_one_shot_mesh(views, one_shot, name):
    """The property of the definition: slots the one-shot would not have hold
    no inside corner, and no active cell reaches into them."""
    box = BOXES[name]
    state = ref.create(*box)
    state["seeds"] = np.ones_like(state["seeds"])
    state = ref.integrate(state, *views, grow=False)
    assert state["slots"].all()
    got = ref.extract(state)
    want = one_shot[name]
    # (the one-shot allocates every brick of the small box: only the deep one decides)
    assert (want["stats"]["allocated_bricks"], got["stats"]["allocated_bricks"]) \
        == {"37x29x23": (120, 120), "61x53x75": (290, 1064)}[name]
    same(got, want, MESH_KEYS + ("cells",))
    assert len(got["faces"]) > 100


# -------------------------------------------------------------------- budget
def test_the_budget_is_checked_before_anything_changes(views):
    first, second = batches_of((4, 1), *views)
    need = ref.stats(ref.mark(ref.create(*DEEP), *views[:2]))
    need = need["allocated_bricks"] + need["pending_bricks"]
    assert need == 290
    state = ref.integrate(ref.create(*DEEP, max_bricks=need - 1), *first)
    with pytest.raises(ref.OverBudget) as e:
        ref.mark(state, *second[:2])
    assert e.value.need == need
    with pytest.raises(ref.OverBudget):
        ref.integrate(state, *second)
    assert ref.stats(state)["allocated_bricks"] == 242


def test_nothing_marked_is_an_empty_mesh():
    got = ref.extract(ref.create(*SMALL))
    assert np.isnan(got["tsdf"]).all() and got["xyz"].shape == (0, 3)
    assert got["faces"].shape == (0, 3) and not got["brick_state"].any()


# ------------------------------------------------------------------ the C ABI
@pytest.fixture(scope="module")
def lib():
    from smvs_amd import build as hip_build, _capi
    hip_build.build()
    lib = _capi.load()
    lib.smvs_last_error.restype = C.c_char_p
    return lib


NAMES = ["smvs_tsdf_sparse_volume_" + n for n in (
    "create", "mark", "integrate", "extract", "info", "download", "upload", "reset", "release")]


def test_entries_are_declared_and_exported(lib):
    import smvs_amd
    from smvs_amd import _capi
    for name in NAMES:
        assert name in _capi.declared_symbols() and hasattr(lib, name), name
    assert smvs_amd.SparseTsdfVolume is smvs_amd.device.SparseTsdfVolume


def volume_options(**changes):
    from smvs_amd import _capi
    values = dict(origin=(-1.0, -1.0, 3.0), voxel_size=0.25, dims=(8, 8, 8), trunc=0.0,
                  max_bricks=0)
    values.update(changes)
    opt = _capi.TsdfSparseVolumeOptions()
    opt.voxel_size = values["voxel_size"]
    opt.trunc = values["trunc"]
    opt.max_bricks = values["max_bricks"]
    for k in range(3):
        opt.origin[k] = values["origin"][k]
        opt.dims[k] = values["dims"][k]
    return opt


CREATE_REFUSED = [
    dict(voxel_size=0.0), dict(voxel_size=-0.1), dict(voxel_size=float("nan")),
    dict(voxel_size=float("inf")),
    dict(dims=(1, 8, 8)), dict(dims=(8, 8, 1)), dict(dims=(8, 4097, 8)), dict(dims=(8, 8, 0)),
    dict(origin=(float("nan"), 0.0, 0.0)), dict(origin=(0.0, 0.0, float("inf"))),
    dict(trunc=float("nan")), dict(max_bricks=(1 << 23) + 1),
]


@pytest.mark.parametrize("case", CREATE_REFUSED,
                         ids=lambda c: ",".join("%s=%s" % kv for kv in c.items()))
def test_create_refusals_are_status_codes(lib, case):
    """Before any device call: the same status with or without a device."""
    opt = volume_options(**case)
    handle = C.c_void_p(1)
    assert lib.smvs_tsdf_sparse_volume_create(0, C.byref(opt), C.byref(handle)) == -1, \
        lib.smvs_last_error()
    assert handle.value is None


def test_other_refusals(lib):
    opt = volume_options()
    handle = C.c_void_p(1)
    assert lib.smvs_tsdf_sparse_volume_create(0, None, C.byref(handle)) == -1
    assert handle.value is None
    assert lib.smvs_tsdf_sparse_volume_create(0, C.byref(opt), None) == -1
    # a NULL volume
    mesh = C.c_void_p(1)
    assert lib.smvs_tsdf_sparse_volume_mark(None, None, 0, 0, 0) == -1
    assert lib.smvs_tsdf_sparse_volume_integrate(None, None, 0, 0, 1, 0) == -1
    assert lib.smvs_tsdf_sparse_volume_extract(None, 0, None, None, None, C.byref(mesh), None,
                                               None) == -1
    assert mesh.value is None
    assert lib.smvs_tsdf_sparse_volume_info(None, None, None, None) == -1
    assert lib.smvs_tsdf_sparse_volume_download(None, None, None, None, None, None, None) == -1
    assert lib.smvs_tsdf_sparse_volume_upload(None, None, None, None, C.c_int64(0), None, None,
                                              None, C.c_int64(0)) == -1
    assert lib.smvs_tsdf_sparse_volume_reset(None) == -1
    lib.smvs_tsdf_sparse_volume_release(None)
    if lib.smvs_device_count() < 1:
        # accepted options reach the device, and without one that is an error
        # of its own, not an argument error
        assert lib.smvs_tsdf_sparse_volume_create(0, C.byref(opt), C.byref(handle)) == -2
        assert handle.value is None


def test_a_closed_volume_is_a_python_error():
    import smvs_amd
    vol = smvs_amd.SparseTsdfVolume.__new__(smvs_amd.SparseTsdfVolume)
    vol._handle = None          # what close() leaves
    for call in (lambda: vol.mark([], [], None), lambda: vol.integrate([], [], None, []),
                 vol.extract, vol.state, vol.stats, vol.reset, lambda: vol.n_views,
                 lambda: vol.load_state(None, None, None, None, None, None, 0), vol.__enter__):
        with pytest.raises(ValueError, match="closed"):
            call()
    vol.close()                 # closing twice is fine
