"""CPU checks of the adaptive-penalty SGM mode: the
serial restatement tests/sgm_adaptive_reference.cc against the pins that are
already in the tree (the oracle's single scalar step, the oracle's constant-P2
aggregation on an image of constant intensity), against a hand-computed case,
and the new C entries' argument checks, which need no GPU."""
import ctypes as C

import numpy as np
import pytest

import sgm_adaptive_ref as ref  # tests/sgm_adaptive_ref.py


# A5's range for the random rows: path costs of a line are <= max(510, 255 + Pmax)
def _random_row(rng, D, pmax):
    prev = rng.integers(0, max(510, 255 + pmax) + 1, D).astype(np.uint16)
    cost = rng.integers(0, 256, D).astype(np.uint16)
    cost[rng.integers(0, D, max(1, D // 16))] = 255
    return prev, cost


@pytest.mark.parametrize("D", [5, 16, 128])
@pytest.mark.parametrize("p1,p2", [(6, 96), (10, 12), (3, 300), (40, 20)])
def test_single_step_equals_the_oracles_scalar_step(oracle, D, p1, p2):
    """1. restatement's step (literal loop) == orc_sgm_path_step_scalar"""
    L = oracle.lib()
    u16 = oracle.c_u16_p
    rng = np.random.default_rng(100 * D + p1)
    pmax = max(p2, p1 * 3 // 2)
    for trial in range(100):
        prev, cost = _random_row(rng, D, pmax)
        i1, i2 = int(rng.integers(0, 256)), int(rng.integers(0, 256))
        if trial % 5 == 0:
            i2 = i1
        want = np.zeros(D, np.uint16)
        L.orc_sgm_path_step_scalar(prev.ctypes.data_as(u16), cost.ctypes.data_as(u16), D,
                                   i1, i2, C.c_uint16(p1), C.c_uint16(p2),
                                   want.ctypes.data_as(u16))
        got = ref.step(prev, cost, i1, i2, p1, p2, literal=True)
        assert np.array_equal(got, want), (trial, i1, i2)
        assert ref.penalty(i1, i2, p1, p2) == max(p1 * 3 // 2, p2 // (abs(i1 - i2) + 1))


@pytest.mark.parametrize("D", [2, 3, 5, 16, 128])
@pytest.mark.parametrize("p1,p2", [(6, 96), (10, 12), (3, 300), (40, 20), (170, 255)])
def test_literal_loop_equals_closed_form(D, p1, p2):
    """2. A2: min over the literal j loop == min(prev[i], prev[i +- 1] + P1,
    min_prev + penalty2') inside A5's range"""
    rng = np.random.default_rng(7 * D + p2)
    pmax = max(p2, p1 * 3 // 2)
    for trial in range(100):
        prev, cost = _random_row(rng, D, pmax)
        i1, i2 = int(rng.integers(0, 256)), int(rng.integers(0, 256))
        a = ref.step(prev, cost, i1, i2, p1, p2, literal=True)
        b = ref.step(prev, cost, i1, i2, p1, p2, literal=False)
        assert np.array_equal(a, b), (trial, i1, i2)


@pytest.mark.parametrize("w,h,D", [(13, 9, 8), (9, 14, 5), (24, 24, 16)])
def test_constant_image_equals_constant_p2_except_on_the_two_a4_diagonals(oracle, w, h, D):
    """3. constant intensity: penalty2' = penalty2 (>= P1 * 3 / 2), so the
    volume is the SSE build's everywhere except on the two diagonals that start
    in the bottom corners (A4), and differs somewhere on them."""
    rng = np.random.default_rng(w * h)
    cost = rng.integers(0, 256, (h, w, D)).astype(np.uint16)
    image = np.full((h, w), 117, np.uint8)
    p1, p2 = 6, 96
    want = oracle.sgm_aggregate(cost, p1, p2)
    for literal in (True, False):
        got = ref.aggregate(cost, image, p1, p2, literal=literal)
        lines = ref.a4_lines(w, h)
        assert lines.sum() <= 2 * min(w, h)
        assert np.array_equal(got[~lines], want[~lines])
        assert not np.array_equal(got[lines], want[lines])
        # the corners themselves hold the same S (A4 changes the path volume
        # there, and S gets 2 C from the corner in both builds)
        assert np.array_equal(got[h - 1, 0], want[h - 1, 0])
        assert np.array_equal(got[h - 1, w - 1], want[h - 1, w - 1])


def test_image_edge_changes_the_far_side():
    """4a. a step edge in the image lowers penalty2' for the steps across it:
    the volume changes on the far side of the edge for the paths that cross it."""
    rng = np.random.default_rng(3)
    w, h, D = 20, 12, 16
    cost = rng.integers(0, 256, (h, w, D)).astype(np.uint16)
    flat = np.full((h, w), 60, np.uint8)
    edge = flat.copy()
    edge[:, 12:] = 200
    a = ref.aggregate(cost, flat, 6, 96)
    b = ref.aggregate(cost, edge, 6, 96)
    changed = (a != b).any(axis=2)
    assert changed[:, 12:].any() and changed[:, :12].any()
    # (both sides: the paths to the right cross the edge into columns >= 12,
    # the paths to the left cross it into columns < 12)
    # A1 on single values: int division, floored at P1 * 3 / 2
    assert ref.penalty(200, 60, 6, 96) == 9 and ref.penalty(60, 60, 6, 96) == 96
    assert ref.penalty(61, 60, 6, 96) == 48 and ref.penalty(60, 255, 6, 96) == 9
    assert ref.penalty(0, 255, 40, 20) == 60 and ref.penalty(9, 9, 40, 20) == 60


def test_hand_computed_3x3x4():
    """4b. 3 x 3 pixels, 4 planes, P1 = 2, P2 = 40.  Image columns 10, 10, 49
    (|dI| + 1 = 40 across the edge: penalty2' = max(3, 1) = 3; 40 elsewhere).
    Cost, the same in every row: columns 0 and 1 A = [0, 20, 20, 20], column 2
    B = [20, 20, 20, 0].  By hand (u = min(L'(d), L'(d +- 1) + 2, min L' + p2')):
      A -> A flat             a1 = [0, 22, 40, 40]
      a1 -> A flat            a5 = [0, 22, 44, 60]   (B columns: mirrored)
      A or a1 or a6 -> B edge b2 = [20, 22, 23, 3]
      B or 2 B -> A edge      a3 = [3, 23, 22, 20]
      a3 -> A flat            a4 = [0, 22, 39, 37]
      2 A -> A flat           a6 = [0, 22, 60, 60]   (A4: the line from the
                                   bottom-left corner; the SSE build has a1)
    Summed over the eight directions with the seeds of A3 / A4:"""
    A = [0, 20, 20, 20]
    B = [20, 20, 20, 0]
    cost = np.array([[A, A, B]] * 3, np.uint16)
    image = np.array([[10, 10, 49]] * 3, np.uint8)
    want = np.array([
        [[0, 186, 242, 254], [6, 172, 228, 240], [220, 208, 188, 6]],
        [[0, 170, 259, 257], [9, 179, 286, 280], [200, 206, 173, 9]],
        [[0, 186, 242, 254], [6, 172, 228, 240], [220, 208, 188, 6]]], np.uint16)
    for literal in (True, False):
        got = ref.aggregate(cost, image, 2, 40, literal=literal)
        assert np.array_equal(got, want), got


def _hip_lib():
    from smvs_amd import _capi
    return _capi.load()


def _run_mode(lib, p1, p2, mode, num_steps=16):
    w, h = 24, 16
    main = np.full((h, w), 90, np.uint8)
    M = np.eye(3, dtype=np.float32).reshape(9)
    t = np.array([-6, 0, 0], np.float32)
    u8 = C.POINTER(C.c_uint8)
    fp = C.POINTER(C.c_float)
    return lib.smvs_sgm_run_mode(0, main.ctypes.data_as(u8), w, h, main.ctypes.data_as(u8),
                                 w, h, M.ctypes.data_as(fp), t.ctypes.data_as(fp),
                                 C.c_float(1.0), C.c_float(8.0), num_steps, C.c_uint16(p1),
                                 C.c_uint16(p2), C.c_int(mode), None, None, None, None)


def _view_mode(lib, p1, p2, mode, raw):
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
            0, main.ctypes.data_as(u8), w, h, 1, arr, ch, 1, 0, 16, C.c_uint16(p1),
            C.c_uint16(p2), C.c_int(mode), depth.ctypes.data_as(fp))
    return lib.smvs_sgm_depth_for_view_mode(
        0, main.ctypes.data_as(u8), w, h, arr, 1, 16, C.c_uint16(p1), C.c_uint16(p2),
        C.c_int(mode), depth.ctypes.data_as(fp))


def test_new_entries_exist_and_refuse_bad_options_without_a_gpu():
    """5. smvs_sgm_run_mode, smvs_sgm_depth_for_view_mode and ..._raw_mode are
    exported and answer SMVS_ERR_INVALID -- before any device call, so also on
    a machine without a GPU -- to an unknown mode and to penalties outside A5's
    range: 8 (255 + max(P2, P1 * 3 / 2)) + 4 * 255 < 65536, i.e.
    max(P2, P1 * 3 / 2) <= 7809."""
    lib = _hip_lib()
    for name in ("smvs_sgm_run_mode", "smvs_sgm_depth_for_view_mode",
                 "smvs_sgm_depth_for_view_raw_mode"):
        assert hasattr(lib, name), name
    INVALID = -1
    calls = [lambda p1, p2, m: _run_mode(lib, p1, p2, m),
             lambda p1, p2, m: _view_mode(lib, p1, p2, m, raw=False),
             lambda p1, p2, m: _view_mode(lib, p1, p2, m, raw=True)]
    for call in calls:
        for mode in (2, -1, 7):
            assert call(6, 96, mode) == INVALID
            assert b"mode" in lib.smvs_last_error()
        assert call(6, 7810, 1) == INVALID        # P2 alone
        assert call(5207, 96, 1) == INVALID       # P1 * 3 / 2 = 7810
        assert b"u16" in lib.smvs_last_error()
    # the constant mode keeps refusing penalty2 < penalty1 (as smvs_sgm_run does)
    assert _run_mode(lib, 40, 20, 0) == INVALID
    assert b"below penalty1" in lib.smvs_last_error()
    # ... and the plane count is still checked in the adaptive mode
    assert _run_mode(lib, 6, 96, 1, num_steps=129) == INVALID
