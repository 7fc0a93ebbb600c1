"""CPU checks of the SGM plane counts above 128 ("plane
counts"): the rule -- 2 .. 128 as before, plus the multiples of 8 from 136 to
256 -- through every entry that takes a plane count, before any device call;
and the yardsticks of tests/test_gpu_sgm_wide.py at 136 and 256 planes: the
oracle's closed form against its literal loop, the adaptive restatement's
closed form against its literal loop."""
import ctypes as C

import numpy as np
import pytest

import sgm_adaptive_ref as ref  # tests/sgm_adaptive_ref.py

INVALID = -1
ACCEPTED = (136, 200, 256)
REFUSED = (130, 132, 255, 257, 264, 512)
RULE = b"multiple of 8 in [136, 256]"


def _hip_lib():
    from smvs_amd import _capi
    return _capi.load()


def _host_lib():
    from smvs_amd import host
    return host.load()


def _run_mode(lib, num_steps, mode):
    w, h = 24, 16
    main = np.full((h, w), 90, np.uint8)
    M = np.eye(3, dtype=np.float32).reshape(9)
    t = np.array([-6, 0, 0], np.float32)
    u8 = C.POINTER(C.c_uint8)
    fp = C.POINTER(C.c_float)
    return lib.smvs_sgm_run_mode(0, main.ctypes.data_as(u8), w, h, main.ctypes.data_as(u8),
                                 w, h, M.ctypes.data_as(fp), t.ctypes.data_as(fp),
                                 C.c_float(1.0), C.c_float(8.0), num_steps, C.c_uint16(6),
                                 C.c_uint16(96), C.c_int(mode), None, None, None, None)


def _view_mode(lib, num_steps, mode, raw):
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
    if raw:
        ch = (C.c_int * 1)(1)
        return lib.smvs_sgm_depth_for_view_raw_mode(
            0, main.ctypes.data_as(u8), w, h, 1, arr, ch, 1, 0, num_steps, C.c_uint16(6),
            C.c_uint16(96), C.c_int(mode), depth.ctypes.data_as(fp))
    return lib.smvs_sgm_depth_for_view_mode(
        0, main.ctypes.data_as(u8), w, h, arr, 1, num_steps, C.c_uint16(6), C.c_uint16(96),
        C.c_int(mode), depth.ctypes.data_as(fp))


CALLS = {
    "run_mode": lambda lib, n, m: _run_mode(lib, n, m),
    "depth_for_view_mode": lambda lib, n, m: _view_mode(lib, n, m, raw=False),
    "depth_for_view_raw_mode": lambda lib, n, m: _view_mode(lib, n, m, raw=True),
}


@pytest.mark.parametrize("entry", sorted(CALLS))
@pytest.mark.parametrize("mode", [0, 1])
def test_plane_count_rule_before_any_device_call(entry, mode):
    """Refused counts are SMVS_ERR_INVALID with the message of the new rule;
    accepted ones get past the rule: with a GPU they run, without one they fail
    later (SMVS_ERR_HIP), never with the plane-count message."""
    lib = _hip_lib()
    call = CALLS[entry]
    for n in REFUSED:
        assert call(lib, n, mode) == INVALID, n
        assert RULE in lib.smvs_last_error(), (n, lib.smvs_last_error())
    for n in ACCEPTED:
        rc = call(lib, n, mode)
        if rc != 0:
            assert rc != INVALID, (n, lib.smvs_last_error())
            assert b"num_steps" not in lib.smvs_last_error(), (n, lib.smvs_last_error())
    # what was refused and accepted below 129 stays so
    assert call(lib, 129, mode) == INVALID and RULE in lib.smvs_last_error()
    assert call(lib, 1, mode) == INVALID and RULE in lib.smvs_last_error()
    assert call(lib, 0, mode) == INVALID
    assert call(lib, -8, mode) == INVALID


def test_host_entries_exist_and_refuse_the_same_counts(tmp_path):
    """smvs_host_sgm_depth_steps and smvs_host_reconstruct_scene_steps: the rule
    is an argument error before anything is read or run."""
    from smvs_amd import host
    hlib = _host_lib()
    assert hasattr(hlib, "smvs_host_sgm_depth_steps")
    assert hasattr(hlib, "smvs_host_reconstruct_scene_steps")
    hlib.smvs_host_last_error.restype = C.c_char_p
    st = host.ReconSettings(b"undistorted", 1.0, 2, 0, 1, 0, 0, 0, 0.0, 0.0, 1, 6, 3, 0, 1, 2,
                            -1, 1700000)
    n = C.c_int(0)
    missing = str(tmp_path / "no_such_scene").encode()
    for steps in REFUSED + (129, 1, 0, -8):
        rc = hlib.smvs_host_sgm_depth_steps(None, None, 0, None, 1, C.c_float(0), C.c_float(0),
                                            0, 0, C.c_int(steps), None, None, None)
        assert rc != 0, steps
        assert RULE in hlib.smvs_host_last_error(), steps
        rc = hlib.smvs_host_reconstruct_scene_steps(missing, C.byref(st), C.c_uint(0),
                                                    C.c_int(steps), None, 0, None, 0,
                                                    C.byref(n), None, None, None)
        assert rc != 0, steps
        assert RULE in hlib.smvs_host_last_error(), steps
    for steps in ACCEPTED + (128, 2, 37):
        # an accepted count gets as far as the scene, which does not exist
        rc = hlib.smvs_host_reconstruct_scene_steps(missing, C.byref(st), C.c_uint(0),
                                                    C.c_int(steps), None, 0, None, 0,
                                                    C.byref(n), None, None, None)
        assert rc != 0
        assert RULE not in hlib.smvs_host_last_error(), steps
    # the Python front passes the count down
    with pytest.raises(Exception) as err:
        host.reconstruct_scene(str(tmp_path / "no_such_scene"), sgm_num_steps=132)
    assert RULE.decode() in str(err.value)


@pytest.mark.parametrize("D", [136, 256])
def test_oracle_closed_form_equals_literal_loop_above_128(oracle, D):
    """The constant-penalty yardstick at the new plane counts: small random
    volume, costs 0 .. 255 with some planes at 255 (not warped)."""
    rng = np.random.default_rng(D)
    w, h = 13, 10
    cost = rng.integers(0, 256, (h, w, D)).astype(np.uint16)
    cost[rng.random((h, w, D)) < 0.05] = 255
    for p1, p2 in ((6, 96), (10, 300), (170, 255)):
        a = oracle.sgm_aggregate(cost, p1, p2, literal=True)
        b = oracle.sgm_aggregate(cost, p1, p2, literal=False)
        assert np.array_equal(a, b), (p1, p2)
        assert a.max() > 8 * 255 // 2


@pytest.mark.parametrize("D", [136, 256])
def test_adaptive_restatement_closed_form_equals_literal_loop_above_128(D):
    rng = np.random.default_rng(1000 + D)
    w, h = 13, 10
    cost = rng.integers(0, 256, (h, w, D)).astype(np.uint16)
    cost[rng.random((h, w, D)) < 0.05] = 255
    image = rng.integers(0, 256, (h, w)).astype(np.uint8)
    for p1, p2 in ((6, 96), (10, 300), (171, 255)):
        a = ref.aggregate(cost, image, p1, p2, literal=True)
        b = ref.aggregate(cost, image, p1, p2, literal=False)
        assert np.array_equal(a, b), (p1, p2)
