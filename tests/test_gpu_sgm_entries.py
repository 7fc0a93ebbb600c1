"""The 14 view and sweep entries of the SGM front end (include/smvs_hip.h:
smvs_sgm_depth_for_view*, smvs_sgm_sweep_for_view*) called directly through
ctypes on the 384 x 256 sphere scene at SGM scale 192 x 128 with 64 planes: the
entries of one front that differ only in the options they fix give the same
bytes and the same launches per kernel class, and the speckle filter of a
*_filtered entry adds its four launches and nothing else."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_NEIGHBORS = 4
PLANES = 64
K_NAMES = ["census", "warp", "cost", "paths", "wta", "lr_check", "merge", "bilateral"]
OFF = (0, 1, 0, 0.95)           # both filters off
SPECKLE = (0, 1, 50, 0.95)      # the speckle filter alone


@pytest.fixture(scope="module")
def scene():
    """(lib, main image, the four neighbours, the main view's depth range)"""
    import smvs_amd
    from smvs_amd import _capi, host, synth
    if smvs_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on a GPU")
    inputs = synth.pipeline_inputs("sphere", 384, 256, N_NEIGHBORS, flen=1.2)
    imgs = [host.sgm_image(inputs, k, 1) for k in range(N_NEIGHBORS + 1)]
    assert imgs[0].shape == (128, 192)
    small = dict(inputs, images=imgs)
    nbs = []
    for k in range(1, N_NEIGHBORS + 1):
        Mf, tf = host.view_reprojection(small, 0, k)
        Mb, tb = host.view_reprojection(small, k, 0)
        nbs.append(dict(image=imgs[k], M_fwd=Mf, t_fwd=tf, M_bwd=Mb, t_bwd=tb,
                        range_main=host.depth_range(inputs, 0),
                        range_neighbor=host.depth_range(inputs, k)))
    return _capi.load(), imgs[0], nbs, nbs[0]["range_main"]


def _call(scene, entry, n, opts=None, mode=None, filt=None, volumes=False):
    """One entry on the scene's first n neighbours; the outputs it has, by name.
    A *_raw entry gets the same SGM-scale images as one channel, no halving."""
    from smvs_amd import device
    from smvs_amd._capi import check
    lib, main, nbs, rng = scene
    u8p, fp, u16p, i32p = (C.POINTER(t) for t in (C.c_uint8, C.c_float, C.c_uint16, C.c_int32))
    h, w = main.shape
    keep = []
    arr = device._sgm_neighbors(nbs[:n], keep)
    sweep, raw = "sweep" in entry, "_raw" in entry
    out = dict(depth=np.zeros((h, w), np.float32))
    a = [0, main.ctypes.data_as(u8p), w, h] + ([1] if raw else []) + [arr] \
        + ([(C.c_int * n)(*[1] * n)] if raw else []) + [n] + ([0] if raw else [])
    if sweep:
        a += [(C.c_float * 2)(float(rng[0]), float(rng[1]))]
    a += [PLANES, C.c_uint16(6), C.c_uint16(96)]
    if mode is not None:
        a += [mode]
    if opts is not None:
        a += [C.byref(opts)]
    if filt is not None:
        f = device.SgmFilterOptions(*filt)
        a += [C.byref(f)]
    a += [out["depth"].ctypes.data_as(fp)]
    if isinstance(opts, device.SgmViewOptions):
        if opts.merge == device.MERGE_CONSENSUS:
            out.update(checked=np.zeros((n, h, w), np.float32), support=np.zeros((h, w), np.uint8))
            a += [out["checked"].ctypes.data_as(fp), out["support"].ctypes.data_as(u8p)]
        else:
            a += [None, None]
    elif sweep:
        out.update(support=np.zeros((h, w), np.uint8))
        if raw:
            a += [out["support"].ctypes.data_as(u8p)]
        else:
            out.update(argmin=np.zeros((h, w), np.int32))
            vol = [None, None]
            if volumes:
                out.update(cost=np.zeros((h, w, PLANES), np.uint16),
                           sgm=np.zeros((h, w, PLANES), np.uint16))
                vol = [out["cost"].ctypes.data_as(u16p), out["sgm"].ctypes.data_as(u16p)]
            a += [out["argmin"].ctypes.data_as(i32p), out["support"].ctypes.data_as(u8p)] + vol
            if filt is not None:
                a += [None]
    check(getattr(lib, entry)(*a))
    return out


def _launches(scene, call):
    """(the outputs, the launches per kernel class) of one call after a warm-up call"""
    lib = scene[0]
    call()
    lib.smvs_sgm_profile(1, None, None)
    try:
        out = call()
    finally:
        cnt = (C.c_longlong * 8)()
        lib.smvs_sgm_profile(0, None, cnt)
    return out, dict(zip(K_NAMES, [int(c) for c in cnt]))


def _same_group(scene, calls, keys):
    """Every call of the group gives the first one's bytes under `keys` (a call
    that lacks a key is not asked for it) and the first one's launches."""
    first = first_cnt = None
    for name, call in calls:
        out, cnt = _launches(scene, call)
        if first is None:
            first, first_cnt = out, cnt
            depth = out["depth"]
            assert (depth != 0).any() and (depth == 0).any(), name
            assert all(k in out for k in keys), name
        for k in keys:
            if k in out:
                assert out[k].tobytes() == first[k].tobytes(), (name, k)
        assert cnt == first_cnt, (name, cnt, first_cnt)
    return first, first_cnt


def _speckle_adds_four_merge_launches(scene, plain, plain_cnt, filtered):
    for name, call in filtered:
        out, cnt = _launches(scene, call)
        assert cnt == dict(plain_cnt, merge=plain_cnt["merge"] + 4), (name, cnt, plain_cnt)
        # the filter only removes
        assert np.all((out["depth"] == plain["depth"]) | (out["depth"] == 0)), name


def test_reference_front_entries_agree(scene):
    """Two neighbours: the plain, _mode (constant), _opts (constant, plane),
    _merge (reference) and _filtered (reference, filters off) entries and their
    five _raw siblings give one and the same depth bytes and launches."""
    from smvs_amd import device
    o = device.SgmOptions(device.P2_CONSTANT, device.WINNER_PLANE)
    v = device.SgmViewOptions(device.P2_CONSTANT, device.WINNER_PLANE, device.MERGE_REFERENCE,
                              2, 0.95)
    calls = []
    for raw in ("", "_raw"):
        base = "smvs_sgm_depth_for_view" + raw
        calls += [(base, lambda e=base: _call(scene, e, 2)),
                  (base + "_mode", lambda e=base + "_mode": _call(scene, e, 2,
                                                                   mode=device.P2_CONSTANT)),
                  (base + "_opts", lambda e=base + "_opts": _call(scene, e, 2, opts=o)),
                  (base + "_merge", lambda e=base + "_merge": _call(scene, e, 2, opts=v)),
                  (base + "_filtered", lambda e=base + "_filtered": _call(scene, e, 2, opts=v,
                                                                           filt=OFF))]
    assert len(calls) == 10
    plain, cnt = _same_group(scene, calls, ("depth",))
    assert cnt["lr_check"] == 2 and cnt["merge"] == 1 and cnt["wta"] == 4
    _speckle_adds_four_merge_launches(scene, plain, cnt, [
        (e, lambda e=e: _call(scene, e, 2, opts=v, filt=SPECKLE))
        for e in ("smvs_sgm_depth_for_view_filtered", "smvs_sgm_depth_for_view_raw_filtered")])


def test_consensus_front_entries_agree(scene):
    """Four neighbours: _merge and _filtered (filters off) and their _raw
    siblings give the same depth, checked and support bytes and launches."""
    from smvs_amd import device
    v = device.SgmViewOptions(device.P2_CONSTANT, device.WINNER_PLANE, device.MERGE_CONSENSUS,
                              2, 0.95)
    calls = []
    for raw in ("", "_raw"):
        base = "smvs_sgm_depth_for_view" + raw
        calls += [(base + "_merge", lambda e=base + "_merge": _call(scene, e, N_NEIGHBORS, opts=v)),
                  (base + "_filtered", lambda e=base + "_filtered": _call(
                      scene, e, N_NEIGHBORS, opts=v, filt=OFF))]
    plain, cnt = _same_group(scene, calls, ("depth", "checked", "support"))
    assert cnt["wta"] == 2 * N_NEIGHBORS and cnt["merge"] == 1 and cnt["lr_check"] == 0
    assert plain["support"].max() == N_NEIGHBORS
    _speckle_adds_four_merge_launches(scene, plain, cnt, [
        (e, lambda e=e: _call(scene, e, N_NEIGHBORS, opts=v, filt=SPECKLE))
        for e in ("smvs_sgm_depth_for_view_filtered", "smvs_sgm_depth_for_view_raw_filtered")])


def test_sweep_front_entries_agree(scene):
    """Four neighbours: smvs_sgm_sweep_for_view and _filtered (filters off) give
    the same depth, argmin, support, cost and sgm bytes; the two _raw forms the
    same depth and support; all four the same launches."""
    from smvs_amd import device
    s = device.SgmSweepOptions(device.P2_CONSTANT, device.WINNER_PLANE,
                               *device.sgm_sweep_defaults(N_NEIGHBORS))
    calls = [("smvs_sgm_sweep_for_view", lambda: _call(
                 scene, "smvs_sgm_sweep_for_view", N_NEIGHBORS, opts=s, volumes=True)),
             ("smvs_sgm_sweep_for_view_filtered", lambda: _call(
                 scene, "smvs_sgm_sweep_for_view_filtered", N_NEIGHBORS, opts=s, filt=OFF,
                 volumes=True)),
             ("smvs_sgm_sweep_for_view_raw", lambda: _call(
                 scene, "smvs_sgm_sweep_for_view_raw", N_NEIGHBORS, opts=s)),
             ("smvs_sgm_sweep_for_view_raw_filtered", lambda: _call(
                 scene, "smvs_sgm_sweep_for_view_raw_filtered", N_NEIGHBORS, opts=s, filt=OFF))]
    plain, cnt = _same_group(scene, calls, ("depth", "argmin", "support", "cost", "sgm"))
    assert cnt["census"] == 1 and cnt["warp"] == N_NEIGHBORS and cnt["wta"] == 1
    assert plain["support"].max() == N_NEIGHBORS
    _speckle_adds_four_merge_launches(scene, plain, cnt, [
        (e, lambda e=e: _call(scene, e, N_NEIGHBORS, opts=s, filt=SPECKLE))
        for e in ("smvs_sgm_sweep_for_view_filtered", "smvs_sgm_sweep_for_view_raw_filtered")])
