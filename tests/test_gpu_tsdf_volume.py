"""smvs_tsdf_volume on the device: the persistent volume fused batch by batch
against the one-shot entry on the device (fuse_tsdf), the one-shot restatement
(tests/tsdf_ref.py) and the restatement with explicit state
(tests/tsdf_volume_ref.py).  Everything is compared by array_equal, the NaN
positions of the field included.  The shapes are test_gpu_tsdf.py's, at which
tests/test_tsdf_volume_cpu.py shows that a batch-local float sum would differ."""
import os

import numpy as np
import pytest

import tsdf_ref  # tests/tsdf_ref.py
import tsdf_volume_ref as ref  # tests/tsdf_volume_ref.py
from test_gpu_tsdf import DIMS, SURFACE_BOX, VOXEL, _cut_maps, _inputs
from test_tsdf_volume_cpu import PARTITIONS, batches_of

pytestmark = pytest.mark.gpu

ALL = ("tsdf", "weight", "xyz", "normals", "rgb", "confidence", "faces")
MESH = ("xyz", "normals", "rgb", "confidence", "faces")


@pytest.fixture(scope="module")
def hip():
    import smvs_amd
    if smvs_amd.device_count() < 1:
        pytest.fail("no HIP device")
    return smvs_amd


def same(got, want, keys=ALL):
    assert set(got) == set(want) or keys is not ALL
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k], equal_nan=(k == "tsdf")), k


def same_state(got, want):
    """(S, W, rgbc) of TsdfVolume.state() against a restated state"""
    for g, k in zip(got, ("S", "W", "rgbc")):
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, k
        assert g.tobytes() == want[k].tobytes(), k


def fused(hip, batches, cut, origin=SURFACE_BOX, voxel=VOXEL, dims=DIMS, trunc=0):
    """a volume with the batches (cams, depths, normals, images) integrated"""
    vol = hip.TsdfVolume(origin, voxel, dims, trunc=trunc)
    for cams, depths, normals, images in batches:
        vol.integrate(cams, depths, normals, images, cut=cut)
    return vol


@pytest.fixture(scope="module")
def views():
    return _inputs(5, 97, 63, 3)     # cams, depths, normals, images


@pytest.fixture(scope="module")
def one_shot(hip, views):
    """the cut off: the device's one-shot and the restatement's, which agree"""
    cams, depths, normals, images = views
    dev = {mw: hip.fuse_tsdf(cams, depths, normals, images, SURFACE_BOX, VOXEL, DIMS, cut=False,
                             volume=True, min_weight=mw) for mw in (1, 2)}
    want = {mw: tsdf_ref.fuse(cams, depths, images, SURFACE_BOX, VOXEL, DIMS, min_weight=mw)
            for mw in (1, 2)}
    for mw in (1, 2):
        same(dev[mw], want[mw])
    return dev


# ---------------------------------------------------------------- the cut off
@pytest.mark.parametrize("partition", PARTITIONS, ids=str)
def test_every_partition_is_the_one_shot(hip, views, one_shot, partition):
    cams, depths, normals, images = views
    with fused(hip, batches_of(partition, *views), cut=False) as vol:
        assert vol.n_views == 5
        got = vol.extract(volume=True)
        state = vol.state()
    same(got, one_shot[1])
    assert np.array_equal(np.isnan(got["tsdf"]), np.isnan(one_shot[1]["tsdf"]))
    assert len(got["faces"]) > 100 and got["faces"].max() < len(got["xyz"])
    want = ref.fuse_batches(batches_of(partition, cams, depths, images), SURFACE_BOX, VOXEL, DIMS)
    same_state(state, want)
    same(got, ref.extract(want))


def test_normals_are_not_needed_without_the_cut(hip, views, one_shot):
    cams, depths, _, images = views
    with hip.TsdfVolume(SURFACE_BOX, VOXEL, DIMS) as vol:
        vol.integrate(cams[:2], depths[:2], None, images[:2], cut=False)
        vol.integrate(cams[2:], depths[2:], None, images[2:], cut=False)
        got = vol.extract()
    assert set(got) == set(MESH)
    same(got, one_shot[1], MESH)


# ----------------------------------------------------------------- the cut on
def test_one_batch_with_the_cut_is_the_one_shot(hip, views):
    cams, depths, normals, images = views
    want = hip.fuse_tsdf(cams, depths, normals, images, SURFACE_BOX, VOXEL, DIMS, cut=True,
                         volume=True)
    with fused(hip, [views], cut=True) as vol:
        same(vol.extract(volume=True), want)


@pytest.mark.parametrize("partition", [(2, 3), (1, 4)], ids=str)
def test_the_cut_acts_within_a_batch(hip, oracle, views, partition):
    cams, depths, normals, images = views
    batches = batches_of(partition, *views)
    # the oracle's cut maps per batch (a batch of one view is not cut), concatenated
    dms = []
    for c, d, n, _ in batches:
        dms += list(_cut_maps(oracle, c, d, n, True))
    assert any(not np.array_equal(a, b) for a, b in zip(dms, depths))
    want = tsdf_ref.fuse(cams, dms, images, SURFACE_BOX, VOXEL, DIMS)    # 5 views
    with fused(hip, batches, cut=True) as vol:
        got = vol.extract(volume=True)
        state = vol.state()
    same(got, want)
    assert len(got["faces"]) > 100
    same_state(state, ref.fuse_batches(batches_of(partition, cams, dms, images), SURFACE_BOX,
                                       VOXEL, DIMS))


# -------------------------------------------------------------- mixed batches
def test_batches_of_other_sizes_and_channels_and_an_explicit_truncation(hip, oracle):
    cams, depths, normals, images = _inputs(5, 97, 63, 3, last_size=(80, 71))
    assert depths[4].shape == (71, 80) != depths[0].shape
    # a grey batch of two, then an RGB batch whose last view has a size of its own
    images = [np.ascontiguousarray(im[..., 1]) for im in images[:2]] + images[2:]
    assert images[0].ndim == 2 and images[2].shape[-1] == 3
    views = (cams, depths, normals, images)
    batches = batches_of((2, 3), *views)
    want_dev = hip.fuse_tsdf(*views, SURFACE_BOX, VOXEL, DIMS, trunc=0.1, cut=False, volume=True)
    want = tsdf_ref.fuse(cams, depths, images, SURFACE_BOX, VOXEL, DIMS, trunc=0.1)
    with fused(hip, batches, cut=False, trunc=0.1) as vol:
        got = vol.extract(volume=True)
    same(got, want_dev)
    same(got, want)
    assert len(got["faces"]) > 100
    # and with the cut, which acts within each batch
    dms = []
    for c, d, n, _ in batches:
        dms += list(_cut_maps(oracle, c, d, n, True))
    with fused(hip, batches, cut=True, trunc=0.1) as vol:
        same(vol.extract(volume=True),
             tsdf_ref.fuse(cams, dms, images, SURFACE_BOX, VOXEL, DIMS, trunc=0.1))


# -------------------------------------------------------------- extract twice
def test_extract_twice_with_another_min_weight(hip, views, one_shot):
    with fused(hip, batches_of((2, 3), *views), cut=False) as vol:
        before = [a.tobytes() for a in vol.state()]
        first = vol.extract(min_weight=1, volume=True)
        between = [a.tobytes() for a in vol.state()]
        second = vol.extract(min_weight=2, volume=True)
        again = vol.extract(volume=True)
        after = [a.tobytes() for a in vol.state()]
        assert vol.n_views == 5
    assert before == between == after
    same(first, one_shot[1])
    same(second, one_shot[2])
    same(again, one_shot[1])
    assert np.isnan(second["tsdf"]).sum() > np.isnan(first["tsdf"]).sum()


# ----------------------------------------------------------------- edge cases
def test_extract_before_any_integrate(hip):
    with hip.TsdfVolume(SURFACE_BOX, VOXEL, DIMS) as vol:
        assert vol.n_views == 0
        got = vol.extract(volume=True)
        S, W, rgbc = vol.state()
    assert got["xyz"].shape == (0, 3) and got["faces"].shape == (0, 3)
    assert got["confidence"].shape == (0,) and got["rgb"].shape == (0, 3)
    assert got["tsdf"].shape == DIMS[::-1] and np.isnan(got["tsdf"]).all()
    assert not got["weight"].any() and not S.any() and not W.any() and not rgbc.any()
    assert rgbc.shape == DIMS[::-1] + (4,)


@pytest.mark.parametrize("label,n_views,channels,partition,origin,voxel,dims", [
    ("2x2x2", 2, 3, (1, 1), (-0.06, -0.06, 2.95), VOXEL, (2, 2, 2)),
    ("camera-inside", 5, 1, (2, 3), (-0.6, -0.5, -0.62), 0.15, (8, 7, 41)),
    ("free-space", 2, 3, (1, 1), (-0.3, -0.2, 1.0), 0.03, (9, 8, 7)),
    ("half-outside", 5, 3, (3, 2), (-1.0, -0.2, 2.8), VOXEL, DIMS)])
def test_boxes(hip, label, n_views, channels, partition, origin, voxel, dims):
    views = _inputs(n_views, 97, 63, channels)
    cams, depths, normals, images = views
    want = hip.fuse_tsdf(*views, origin, voxel, dims, cut=False, volume=True)
    with fused(hip, batches_of(partition, *views), False, origin, voxel, dims) as vol:
        got = vol.extract(volume=True)
        state = vol.state()
    same(got, want)
    same(got, tsdf_ref.fuse(cams, depths, images, origin, voxel, dims))
    same_state(state, ref.fuse_batches(batches_of(partition, cams, depths, images), origin,
                                       voxel, dims))
    if label == "2x2x2":
        assert len(got["xyz"]) == 1 and len(got["faces"]) == 0
    if label == "camera-inside":
        centre = np.asarray(cams[1].center)
        assert np.all(centre > origin)
        assert np.all(centre < np.asarray(origin) + voxel * np.array(dims))
        assert np.all(got["weight"][:4] == 0) and len(got["faces"]) > 0
    if label == "free-space":
        assert got["xyz"].shape == (0, 3) and got["faces"].shape == (0, 3)
        assert got["weight"].max() > 0 and np.nanmin(got["tsdf"]) == 1.0
    if label == "half-outside":
        assert np.isnan(got["tsdf"])[:, -3:, :].all() and len(got["faces"]) > 100


# ------------------------------------------------------------ no contribution
def test_a_batch_that_contributes_nothing(hip, views, one_shot):
    cams, depths, normals, images = views
    blind = [np.zeros_like(d) for d in depths[:2]]      # no valid pixel: D == 0 everywhere
    with fused(hip, batches_of((2, 3), *views), cut=False) as vol:
        before = [a.tobytes() for a in vol.state()]
        vol.integrate(cams[:2], blind, normals[:2], images[:2], cut=False)
        assert vol.n_views == 7
        assert [a.tobytes() for a in vol.state()] == before
        got = vol.extract(volume=True)
    # the sums are the 5 views', the confidences follow the 7
    same(got, one_shot[1], [k for k in ALL if k != "confidence"])
    seven = (cams + cams[:2], depths + blind, images + images[:2])
    same(got, tsdf_ref.fuse(*seven, SURFACE_BOX, VOXEL, DIMS))
    same(got, hip.fuse_tsdf(seven[0], seven[1], None, seven[2], SURFACE_BOX, VOXEL, DIMS,
                            cut=False, volume=True))
    assert (got["confidence"] < one_shot[1]["confidence"]).all()


# ------------------------------------------------- checkpoint, reset, volumes
def test_checkpoint_continues_to_the_same_bits(hip, views, one_shot):
    first, second = batches_of((2, 3), *views)
    with fused(hip, [first], cut=False) as vol:
        S, W, rgbc = vol.state()
        n = vol.n_views
    assert n == 2
    with hip.TsdfVolume(SURFACE_BOX, VOXEL, DIMS) as vol:
        vol.load_state(S, W, rgbc, n)
        assert vol.n_views == 2
        same_state(vol.state(), dict(S=S, W=W, rgbc=rgbc))
        vol.integrate(*second, cut=False)
        assert vol.n_views == 5
        resumed = vol.extract(volume=True)
        state = vol.state()
    same(resumed, one_shot[1])
    with fused(hip, [first, second], cut=False) as vol:
        same_state(state, dict(zip(("S", "W", "rgbc"), vol.state())))
    with pytest.raises(ValueError):
        with hip.TsdfVolume(SURFACE_BOX, VOXEL, (8, 8, 8)) as vol:
            vol.load_state(S, W, rgbc, n)


def test_reset(hip, views, one_shot):
    with fused(hip, batches_of((1, 4), *views), cut=False) as vol:
        vol.reset()
        assert vol.n_views == 0
        assert not any(a.any() for a in vol.state())
        assert np.isnan(vol.extract(volume=True)["tsdf"]).all()
        for batch in batches_of((3, 2), *views):
            vol.integrate(*batch, cut=False)
        assert vol.n_views == 5
        same(vol.extract(volume=True), one_shot[1])


def test_two_volumes_side_by_side(hip, views, one_shot):
    other = ((-1.0, -0.2, 2.8), 0.07, (31, 37, 19))
    want_other = hip.fuse_tsdf(*views, *other, cut=False, volume=True)
    a = hip.TsdfVolume(SURFACE_BOX, VOXEL, DIMS)
    b = hip.TsdfVolume(*other)
    try:
        first, second = batches_of((2, 3), *views)
        a.integrate(*first, cut=False)
        b.integrate(*first, cut=False)
        got_half = b.extract(volume=True)
        a.integrate(*second, cut=False)
        same(a.extract(volume=True), one_shot[1])
        b.integrate(*second, cut=False)
        same(b.extract(volume=True), want_other)
        same(a.extract(volume=True), one_shot[1])
        same(got_half, hip.fuse_tsdf(*first, *other, cut=False, volume=True))
    finally:
        a.close()
        b.close()
    with pytest.raises(ValueError, match="closed"):
        a.extract()


# ------------------------------------------------------------------- refusals
def test_refusals_leave_the_volume_usable(hip, views, one_shot):
    import ctypes as C
    from smvs_amd import _capi
    from smvs_amd._capi import SmvsError
    from smvs_amd.device import _tsdf_views
    cams, depths, normals, images = views
    first, second = batches_of((2, 3), *views)

    def refused(call):
        with pytest.raises(SmvsError) as e:
            call()
        assert e.value.status == -1

    refused(lambda: hip.TsdfVolume(SURFACE_BOX, 0.0, DIMS))
    refused(lambda: hip.TsdfVolume(SURFACE_BOX, VOXEL, (37, 1, 23)))
    refused(lambda: hip.TsdfVolume(SURFACE_BOX, VOXEL, (37, 1025, 23)))
    refused(lambda: hip.TsdfVolume(SURFACE_BOX, VOXEL, (1024, 1024, 129)))
    refused(lambda: hip.TsdfVolume((0.0, float("nan"), 0.0), VOXEL, DIMS))
    refused(lambda: hip.TsdfVolume(SURFACE_BOX, VOXEL, DIMS, trunc=float("inf")))
    lib = _capi.load()
    with fused(hip, [first], cut=False) as vol:
        before = [a.tobytes() for a in vol.state()]
        S, W, rgbc = vol.state()
        # what check_views refuses
        refused(lambda: vol.integrate([], [], [], [], cut=False))
        refused(lambda: vol.integrate(*second[:2], None, second[3], cut=True))
        arr, _keep = _tsdf_views(*second)
        for change in ("channels", "image", "depth"):
            arr, _keep = _tsdf_views(*second)
            if change == "channels":
                arr[1].channels = 5
            else:
                setattr(arr[1], change, None)
            assert lib.smvs_tsdf_volume_integrate(vol._handle, arr, 3, 0) == -1, change
        assert lib.smvs_tsdf_volume_integrate(vol._handle, arr, 4097, 0) == -1
        # the view count: 2^24 in all
        refused(lambda: vol.load_state(S, W, rgbc, -1))
        refused(lambda: vol.load_state(S, W, rgbc, (1 << 24) + 1))
        assert lib.smvs_tsdf_volume_upload(vol._handle, None, None, None, C.c_int64(2)) == -1
        assert vol.n_views == 2 and [a.tobytes() for a in vol.state()] == before
        vol.load_state(S, W, rgbc, (1 << 24) - 2)
        refused(lambda: vol.integrate(*second, cut=False))
        assert vol.n_views == (1 << 24) - 2
        vol.load_state(S, W, rgbc, 2)
        assert [a.tobytes() for a in vol.state()] == before
        # no handle pointer
        assert lib.smvs_tsdf_volume_extract(vol._handle, 0, None, None, None, None, None) == -1
        # and the volume goes on as if nothing had been asked
        vol.integrate(*second, cut=False)
        assert vol.n_views == 5
        same(vol.extract(volume=True), one_shot[1])


# ---------------------------------------------------------------- scene entry
@pytest.fixture(scope="module")
def scene(hip, tmp_path_factory):
    """a scene written and reconstructed as test_scene_fused_end_to_end does"""
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
    ("aabb", dict(voxel_size=np.float32(0.05), aabb=AABB)),
    ("clean", dict(resolution=64, clean=dict(percentile=10, component_size=50)))])
def test_scene_batched_is_the_one_shot_file(hip, scene, label, options):
    from smvs_amd import host
    results = {}
    for batch_views in (0, 2, 1):
        out = host.generate_fused(scene, input_scale=0, cut=False, batch_views=batch_views,
                                  **options)
        with open(out[0], "rb") as f:
            results[batch_views] = (os.path.basename(out[0]),) + tuple(out[1:]) + (f.read(),)
        os.remove(out[0])
    name, nv, nf = results[0][:3]
    assert name == ("smvs-clean-B0.ply" if label == "clean" else "smvs-fused-B0.ply")
    assert nf > 100 and len(results[0][-1]) > 1000
    assert results[2] == results[0] and results[1] == results[0]


def test_scene_batches_belong_to_the_dense_volume(hip, scene):
    from smvs_amd import host
    from smvs_amd._capi import SmvsError
    with pytest.raises(SmvsError, match="batch_views belongs to the dense volume"):
        host.generate_fused(scene, resolution=64, input_scale=0, cut=False, sparse=True,
                            batch_views=2)
    with pytest.raises(SmvsError, match="batch_views"):
        host.generate_fused(scene, resolution=64, input_scale=0, cut=False, batch_views=-1)
    # the cut, when on, acts within a batch: one batch of all views is the one-shot
    a = host.generate_fused(scene, resolution=64, input_scale=0, cut=True, batch_views=3)
    with open(a[0], "rb") as f:
        batched = f.read()
    b = host.generate_fused(scene, resolution=64, input_scale=0, cut=True)
    with open(b[0], "rb") as f:
        assert f.read() == batched and a == b
