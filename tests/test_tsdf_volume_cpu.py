"""The persistent fusion volume on the CPU: the numpy restatement with explicit
state (tests/tsdf_volume_ref.py) against the one-shot restatement
(tests/tsdf_ref.py) for every split of the suite's 5 sphere views into
consecutive batches, the proof that these shapes tell the right order of the
float sum from the wrong one, and the refusals of the C ABI, which come before
any device call."""
import ctypes as C

import numpy as np
import pytest

import tsdf_ref  # tests/tsdf_ref.py
import tsdf_volume_ref as ref  # tests/tsdf_volume_ref.py
from test_gpu_tsdf import DIMS, SURFACE_BOX, VOXEL, _inputs  # the suite's fusion inputs

PARTITIONS = [(5,), (1, 4), (2, 3), (3, 2), (1, 1, 1, 1, 1)]
TWO_BATCHES = [(1, 4), (2, 3), (3, 2)]
MESH_KEYS = ("xyz", "normals", "rgb", "confidence", "faces")


def batches_of(partition, *lists):
    """the lists cut into consecutive batches of the partition's sizes"""
    out, at = [], 0
    for n in partition:
        out.append(tuple(x[at:at + n] for x in lists))
        at += n
    assert at == len(lists[0])
    return out


@pytest.fixture(scope="module")
def views():
    cams, depths, _, images = _inputs(5, 97, 63, 3)
    return cams, depths, images       # the cut is off: the maps are the depth maps


@pytest.fixture(scope="module")
def one_shot(views):
    cams, depths, images = views
    F, W, col = tsdf_ref.field(cams, depths, images, SURFACE_BOX, VOXEL, DIMS)
    out = tsdf_ref.fuse(cams, depths, images, SURFACE_BOX, VOXEL, DIMS)
    assert np.array_equal(out["tsdf"], F, equal_nan=True)
    return out, col


@pytest.mark.parametrize("partition", PARTITIONS, ids=str)
def test_every_partition_is_the_one_shot(views, one_shot, partition):
    want, col = one_shot
    state = ref.fuse_batches(batches_of(partition, *views), SURFACE_BOX, VOXEL, DIMS)
    assert state["n_views"] == 5
    assert np.array_equal(state["W"], want["weight"])
    assert np.array_equal(state["rgbc"], col)
    got = ref.extract(state)
    assert np.array_equal(np.isnan(got["tsdf"]), np.isnan(want["tsdf"]))
    assert np.array_equal(got["tsdf"], want["tsdf"], equal_nan=True)
    for k in MESH_KEYS + ("weight",):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    assert len(got["faces"]) > 100
    # and with another min_weight from the same state
    want2 = tsdf_ref.fuse(*views, SURFACE_BOX, VOXEL, DIMS, min_weight=2)
    got2 = ref.extract(state, 2)
    assert np.array_equal(got2["tsdf"], want2["tsdf"], equal_nan=True)
    for k in MESH_KEYS:
        assert np.array_equal(got2[k], want2[k]), k


@pytest.mark.parametrize("partition", TWO_BATCHES, ids=str)
def test_the_batch_local_sum_is_another_sum(views, partition):
    batches = batches_of(partition, *views)
    right = ref.fuse_batches(batches, SURFACE_BOX, VOXEL, DIMS)
    wrong = ref.fuse_batches(batches, SURFACE_BOX, VOXEL, DIMS, batch_local=True)
    assert np.array_equal(right["W"], wrong["W"]) and np.array_equal(right["rgbc"], wrong["rgbc"])
    n_s = int((right["S"] != wrong["S"]).sum())
    Fr, Fw = ref.field(right), ref.field(wrong)
    n_f = int(((Fr != Fw) & ~np.isnan(Fr)).sum())
    print("TSDF-VOLUME batch-local %s: S differs at %d voxels, F at %d" % (partition, n_s, n_f))
    assert n_s > 0 and n_f > 0


def test_a_last_batch_of_one_view_cannot_tell(views):
    # (S0 + (a)) is (S0 + a): why [4, 1] is not among the deciding splits
    batches = batches_of((4, 1), *views)
    right = ref.fuse_batches(batches, SURFACE_BOX, VOXEL, DIMS)
    wrong = ref.fuse_batches(batches, SURFACE_BOX, VOXEL, DIMS, batch_local=True)
    assert np.array_equal(right["S"], wrong["S"])


@pytest.mark.parametrize("partition", TWO_BATCHES, ids=str)
def test_the_splits_touch_voxels_in_every_way(views, partition):
    first, second = batches_of(partition, *views)
    empty = ref.create(SURFACE_BOX, VOXEL, DIMS)
    a = ref.integrate(empty, *first)["W"] > 0
    b = ref.integrate(empty, *second)["W"] > 0
    both, only_a, only_b, neither = (int(x.sum()) for x in (a & b, a & ~b, ~a & b, ~a & ~b))
    print("TSDF-VOLUME touched %s: both %d, first only %d, second only %d, neither %d"
          % (partition, both, only_a, only_b, neither))
    assert both >= 1000 and only_a > 0 and only_b > 0 and neither > 0


def test_integrate_leaves_its_argument_alone(views):
    first, second = batches_of((2, 3), *views)
    s1 = ref.integrate(ref.create(SURFACE_BOX, VOXEL, DIMS), *first)
    keep = {k: s1[k].copy() for k in ("S", "W", "rgbc")}
    s2 = ref.integrate(s1, *second)
    assert s1["n_views"] == 2 and s2["n_views"] == 5
    for k in keep:
        assert np.array_equal(s1[k], keep[k]) and not np.array_equal(s2[k], keep[k]), k


def test_nothing_integrated_is_an_empty_mesh():
    got = ref.extract(ref.create(SURFACE_BOX, VOXEL, DIMS))
    assert np.isnan(got["tsdf"]).all() and got["xyz"].shape == (0, 3)
    assert got["faces"].shape == (0, 3)


# ------------------------------------------------------------------ the C ABI
@pytest.fixture(scope="module")
def lib():
    from smvs_amd import build as hip_build, _capi
    hip_build.build()
    lib = _capi.load()
    lib.smvs_last_error.restype = C.c_char_p
    return lib


NAMES = ["smvs_tsdf_volume_create", "smvs_tsdf_volume_integrate", "smvs_tsdf_volume_extract",
         "smvs_tsdf_volume_info", "smvs_tsdf_volume_download", "smvs_tsdf_volume_upload",
         "smvs_tsdf_volume_reset", "smvs_tsdf_volume_release"]


def test_entries_are_declared_and_exported(lib):
    import smvs_amd
    from smvs_amd import _capi
    for name in NAMES:
        assert name in _capi.declared_symbols() and hasattr(lib, name), name
    assert smvs_amd.TsdfVolume is smvs_amd.device.TsdfVolume


def volume_options(**changes):
    from smvs_amd import _capi
    values = dict(origin=(-1.0, -1.0, 3.0), voxel_size=0.25, dims=(8, 8, 8), trunc=0.0)
    values.update(changes)
    opt = _capi.TsdfVolumeOptions()
    opt.voxel_size = values["voxel_size"]
    opt.trunc = values["trunc"]
    for k in range(3):
        opt.origin[k] = values["origin"][k]
        opt.dims[k] = values["dims"][k]
    return opt


CREATE_REFUSED = [
    dict(voxel_size=0.0), dict(voxel_size=-0.1), dict(voxel_size=float("nan")),
    dict(voxel_size=float("inf")),
    dict(dims=(1, 8, 8)), dict(dims=(8, 8, 1)), dict(dims=(8, 1025, 8)), dict(dims=(8, 8, 0)),
    dict(dims=(1024, 1024, 1024)), dict(dims=(1024, 1024, 129)),
    dict(origin=(float("nan"), 0.0, 0.0)), dict(origin=(0.0, 0.0, float("inf"))),
    dict(trunc=float("nan")),
]


@pytest.mark.parametrize("case", CREATE_REFUSED,
                         ids=lambda c: ",".join("%s=%s" % kv for kv in c.items()))
def test_create_refusals_are_status_codes(lib, case):
    """Before any device call: the same status with or without a device."""
    opt = volume_options(**case)
    handle = C.c_void_p(1)
    assert lib.smvs_tsdf_volume_create(0, C.byref(opt), C.byref(handle)) == -1, \
        lib.smvs_last_error()
    assert handle.value is None


def test_other_refusals(lib):
    opt = volume_options()
    handle = C.c_void_p(1)
    assert lib.smvs_tsdf_volume_create(0, None, C.byref(handle)) == -1 and handle.value is None
    assert lib.smvs_tsdf_volume_create(0, C.byref(opt), None) == -1
    # a NULL volume
    mesh = C.c_void_p(1)
    n = C.c_int64(-7)
    assert lib.smvs_tsdf_volume_integrate(None, None, 0, 0) == -1
    assert lib.smvs_tsdf_volume_extract(None, 0, None, None, C.byref(mesh), None, None) == -1
    assert mesh.value is None
    assert lib.smvs_tsdf_volume_info(None, None, C.byref(n), None) == -1 and n.value == -7
    assert lib.smvs_tsdf_volume_download(None, None, None, None) == -1
    assert lib.smvs_tsdf_volume_upload(None, None, None, None, C.c_int64(0)) == -1
    assert lib.smvs_tsdf_volume_reset(None) == -1
    lib.smvs_tsdf_volume_release(None)
    if lib.smvs_device_count() < 1:
        # accepted options reach the device, and without one that is an error
        # of its own, not an argument error
        assert lib.smvs_tsdf_volume_create(0, C.byref(opt), C.byref(handle)) == -2
        assert handle.value is None


def test_a_closed_volume_is_a_python_error():
    import smvs_amd
    vol = smvs_amd.TsdfVolume.__new__(smvs_amd.TsdfVolume)
    vol._handle = None          # what close() leaves
    for call in (lambda: vol.integrate([], [], None, []), vol.extract, vol.state, vol.reset,
                 lambda: vol.n_views, lambda: vol.load_state(None, None, None, 0),
                 vol.__enter__):
        with pytest.raises(ValueError, match="closed"):
            call()
    vol.close()                 # closing twice is fine
