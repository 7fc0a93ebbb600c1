"""CPU checks of the sub-plane winner of the SGM front end (DESIGN.md section
3.6, "sub-plane depth"): the numpy restatement tests/sgm_subplane_ref.py against
the oracle's plane depths and its integer winner, the properties of the offset,
and the argument checks of the three `_opts` entries, which need no GPU."""
import ctypes as C

import numpy as np
import pytest

import sgm_subplane_ref as ref  # tests/sgm_subplane_ref.py

F = np.float32
INVALID = -1


@pytest.mark.parametrize("D", [33, 64, 128, 200, 256])
@pytest.mark.parametrize("lo,hi", [(1, 12), (3, 12), (1, 6), (0.5, 4)])
def test_inverse_depth_table_gives_the_oracles_depths_bit_for_bit(oracle, D, lo, hi):
    """1. 1 / inv_table == oracle.sgm_depths"""
    inv = ref.inv_table(lo, hi, D)
    assert inv.dtype == F
    assert np.array_equal((F(1.0) / inv).astype(F), oracle.sgm_depths(lo, hi, D))
    assert np.all(np.diff(inv) > 0)


VOLUMES = {}


def _volume(oracle, D, lo, hi):
    """Oracle volume S, its winners and its integer depth map for the pair of
    the GPU test, computed once."""
    key = (D, lo, hi)
    if key not in VOLUMES:
        main, nbr, M, t = ref.scene_pair()
        depths = oracle.sgm_depths(lo, hi, D)
        S = oracle.sgm_aggregate(oracle.sgm_cost_volume(main, nbr, M, t, depths), 6, 96)
        depth, argmin = oracle.sgm_depth_from_volume(S, main, depths)
        for a in (S, depth, argmin):
            a.setflags(write=False)
        VOLUMES[key] = (main, depths, S, depth, argmin)
    return VOLUMES[key]


CASES = [(128, 3, 12), (256, 1, 12), (33, 1, 12), (64, 1, 6)]


@pytest.mark.parametrize("D,lo,hi", CASES)
def test_no_offset_is_the_oracles_depth_and_the_zero_set_is_its(oracle, D, lo, hi):
    """2. subplane_depth == oracle.sgm_depth_from_volume wherever off == 0; the
    same zero set everywhere"""
    main, depths, S, depth, argmin = _volume(oracle, D, lo, hi)
    sub = ref.subplane_depth(S, argmin, main, lo, hi)
    off = ref.winner_offsets(S, argmin)[0]
    assert sub.dtype == F
    assert np.array_equal(sub == 0, depth == 0)
    still = off == 0
    assert (still & (depth > 0)).sum() >= 1 and (~still & (depth > 0)).sum() >= 1
    assert np.array_equal(sub[still], depth[still])
    assert (sub != depth).sum() > 0.5 * (depth > 0).sum()


@pytest.mark.parametrize("D,lo,hi", CASES)
def test_offset_is_at_most_half_a_plane_towards_the_lower_neighbour(oracle, D, lo, hi):
    """3. den >= 0 and |off| <= 0.5 on every valid pixel; the result lies
    between depths[i] and depths[n]"""
    main, depths, S, depth, argmin = _volume(oracle, D, lo, hi)
    off, den, n = ref.winner_offsets(S, argmin)
    sub = ref.subplane_depth(S, argmin, main, lo, hi)
    v = depth > 0
    assert v.sum() > 1000
    assert np.all(den[v] >= 0)
    assert np.all(np.abs(off[v]) <= 0.5)
    i = argmin[v]
    assert np.all((n[v] == i - 1) | (n[v] == i + 1))
    assert np.all(n[v] <= D - 1)
    a, b = depths[i], depths[n[v]]
    assert np.all(sub[v] >= np.minimum(a, b)) and np.all(sub[v] <= np.maximum(a, b))
    # the neighbour is the one with the lower S (towards which the parabola leans)
    moved = v & (off != 0)
    Sl = np.asarray(S, np.int64)
    ii = argmin[moved].astype(np.int64)
    rows = Sl[moved]
    left, right = rows[np.arange(ii.size), ii - 1], rows[np.arange(ii.size), ii + 1]
    assert np.all((n[moved] == ii + 1) == (right < left))


def _hip_lib():
    from smvs_amd import _capi
    return _capi.load()


def _options(p2_mode, winner):
    from smvs_amd.device import SgmOptions
    return SgmOptions(p2_mode, winner)


def _run_opts(lib, opts, p1=6, p2=96, num_steps=16):
    w, h = 24, 16
    main = np.full((h, w), 90, np.uint8)
    M = np.eye(3, dtype=np.float32).reshape(9)
    t = np.array([-6, 0, 0], np.float32)
    u8 = C.POINTER(C.c_uint8)
    fp = C.POINTER(C.c_float)
    return lib.smvs_sgm_run_opts(0, main.ctypes.data_as(u8), w, h, main.ctypes.data_as(u8),
                                 w, h, M.ctypes.data_as(fp), t.ctypes.data_as(fp),
                                 C.c_float(1.0), C.c_float(8.0), num_steps, C.c_uint16(p1),
                                 C.c_uint16(p2), C.byref(opts) if opts is not None else None,
                                 None, None, None, None)


def _view_opts(lib, opts, raw, p1=6, p2=96, num_steps=16):
    from smvs_amd.device import SgmNeighbor
    w, h = 24, 16
    main = np.full((h, w), 90, np.uint8)
    arr = (SgmNeighbor * 1)()
    arr[0].image = main.ctypes.data_as(C.POINTER(C.c_uint8))
    arr[0].width, arr[0].height = w, h
    for i in range(9):
        arr[0].M_fwd[i] = arr[0].M_bwd[i] = float(i % 4 == 0)
    arr[0].t_fwd[0], arr[0].t_bwd[0] = -6.0, 6.0
    arr[0].range_main[0] = arr[0].range_neighbor[0] = 1.0
    arr[0].range_main[1] = arr[0].range_neighbor[1] = 8.0
    depth = np.zeros((h, w), np.float32)
    u8 = C.POINTER(C.c_uint8)
    fp = C.POINTER(C.c_float)
    po = C.byref(opts) if opts is not None else None
    if raw:
        ch = (C.c_int * 1)(1)
        return lib.smvs_sgm_depth_for_view_raw_opts(
            0, main.ctypes.data_as(u8), w, h, 1, arr, ch, 1, 0, num_steps, C.c_uint16(p1),
            C.c_uint16(p2), po, depth.ctypes.data_as(fp))
    return lib.smvs_sgm_depth_for_view_opts(
        0, main.ctypes.data_as(u8), w, h, arr, 1, num_steps, C.c_uint16(p1), C.c_uint16(p2),
        po, depth.ctypes.data_as(fp))


def test_opts_entries_exist_and_refuse_bad_options_without_a_gpu():
    """4. smvs_sgm_run_opts, smvs_sgm_depth_for_view_opts and ..._raw_opts are
    exported and answer SMVS_ERR_INVALID -- before any device call, so also on
    a machine without a GPU -- to an unknown winner and to NULL options, and
    with winner = 1 to a bad plane count, bad penalties and an unknown penalty2
    mode."""
    from smvs_amd import _capi
    lib = _hip_lib()
    for name in ("smvs_sgm_run_opts", "smvs_sgm_depth_for_view_opts",
                 "smvs_sgm_depth_for_view_raw_opts"):
        assert name in _capi.declared_symbols() and hasattr(lib, name), name
    calls = [lambda o, **kw: _run_opts(lib, o, **kw),
             lambda o, **kw: _view_opts(lib, o, raw=False, **kw),
             lambda o, **kw: _view_opts(lib, o, raw=True, **kw)]
    for call in calls:
        for winner in (2, -1):
            for p2_mode in (0, 1):
                assert call(_options(p2_mode, winner)) == INVALID
                assert b"winner" in lib.smvs_last_error()
        assert call(None) == INVALID
        assert b"winner" in lib.smvs_last_error()
        for p2_mode in (2, -1, 7):
            assert call(_options(p2_mode, 1)) == INVALID
            assert b"mode" in lib.smvs_last_error()
        for steps in (129, 132, 1, 0, 264):
            assert call(_options(0, 1), num_steps=steps) == INVALID
            assert b"multiple of 8 in [136, 256]" in lib.smvs_last_error()
        assert call(_options(1, 1), p2=7810) == INVALID        # P2 alone
        assert b"u16" in lib.smvs_last_error()
        assert call(_options(1, 1), p1=5207) == INVALID        # P1 * 3 / 2 = 7810
        assert b"u16" in lib.smvs_last_error()
    # the constant mode keeps refusing penalty2 < penalty1
    assert _run_opts(lib, _options(0, 1), p1=40, p2=20) == INVALID
    assert b"below penalty1" in lib.smvs_last_error()


def test_host_options_default_to_off():
    """5. SGMStereo::Options::subplane and ReconSettings::sgm_subplane (and the
    adaptive penalty beside them) are off in default-constructed settings; the
    Python fronts default to off as well"""
    import inspect
    from smvs_amd import device, host
    hlib = host.load()
    for name in ("smvs_host_sgm_depth_subplane", "smvs_host_reconstruct_scene_subplane"):
        assert hasattr(hlib, name), name
    out = (C.c_int * 4)(7, 7, 7, 7)
    assert hlib.smvs_host_sgm_default_switches(out) == 0
    assert list(out) == [0, 0, 0, 0]
    assert hlib.smvs_host_sgm_default_switches(None) != 0
    for fn, key in ((device.sgm_run, "subplane"), (device.sgm_depth_for_view, "subplane"),
                    (host.sgm_depth, "subplane"), (host.reconstruct_scene, "sgm_subplane")):
        assert inspect.signature(fn).parameters[key].default is False, fn
    # the scene entry checks the plane count first, then reaches the scene
    st = host.ReconSettings(b"undistorted", 1.0, 2, 0, 1, 0, 0, 0, 0.0, 0.0, 1, 6, 3, 0, 1, 2,
                            -1, 1700000)
    n = C.c_int(0)
    hlib.smvs_host_last_error.restype = C.c_char_p
    rc = hlib.smvs_host_reconstruct_scene_subplane(b"/nonexistent", C.byref(st), C.c_uint(0),
                                                   C.c_int(132), C.c_int(1), None, 0, None, 0,
                                                   C.byref(n), None, None, None)
    assert rc != 0 and b"multiple of 8 in [136, 256]" in hlib.smvs_host_last_error()
    rc = hlib.smvs_host_reconstruct_scene_subplane(b"/nonexistent", C.byref(st), C.c_uint(0),
                                                   C.c_int(128), C.c_int(1), None, 0, None, 0,
                                                   C.byref(n), None, None, None)
    assert rc != 0 and b"multiple of 8" not in hlib.smvs_host_last_error()
