"""ctypes front of tests/sgm_adaptive_reference.cc, the serial CPU restatement
of the adaptive-penalty SGM aggregation:
compiled once per session with g++ -O2 into a temporary directory."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None
_u16p = C.POINTER(C.c_uint16)
_u8p = C.POINTER(C.c_uint8)


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="sgm_adaptive_ref_"),
                           "libsgm_adaptive_ref.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-o", out,
                               os.path.join(HERE, "sgm_adaptive_reference.cc")])
        _lib = C.CDLL(out)
        _lib.sgm_adaptive_ref_penalty.restype = C.c_uint16
        _lib.sgm_adaptive_ref_step.restype = None
        _lib.sgm_adaptive_ref_aggregate.restype = None
    return _lib


def penalty(i1, i2, p1, p2):
    """A1: penalty2' of a pixel of intensity i1 whose predecessor has i2."""
    return int(lib().sgm_adaptive_ref_penalty(int(i1), int(i2), C.c_uint16(p1), C.c_uint16(p2)))


def step(prev, cost, i1, i2, p1, p2, literal=True):
    """A2: one step of a path -> L[D] (uint16)."""
    prev = np.ascontiguousarray(prev, np.uint16)
    cost = np.ascontiguousarray(cost, np.uint16)
    out = np.zeros(len(prev), np.uint16)
    lib().sgm_adaptive_ref_step(prev.ctypes.data_as(_u16p), cost.ctypes.data_as(_u16p),
                                len(prev), int(i1), int(i2), C.c_uint16(p1), C.c_uint16(p2),
                                1 if literal else 0, out.ctypes.data_as(_u16p))
    return out


def aggregate(cost, image, p1, p2, literal=True):
    """A1-A5: cost (h, w, D) uint16 holding u8 values, image (h, w) uint8 ->
    S (h, w, D) uint16."""
    cost = np.ascontiguousarray(cost, np.uint16)
    image = np.ascontiguousarray(image, np.uint8)
    h, w, d = cost.shape
    assert image.shape == (h, w)
    out = np.zeros((h, w, d), np.uint16)
    lib().sgm_adaptive_ref_aggregate(cost.ctypes.data_as(_u16p), image.ctypes.data_as(_u8p),
                                     w, h, d, C.c_uint16(p1), C.c_uint16(p2),
                                     1 if literal else 0, out.ctypes.data_as(_u16p))
    return out


def a4_lines(w, h):
    """The pixels of the two diagonals that start in the bottom corners (A4):
    a boolean (h, w) mask of at most 2 * min(w, h) pixels."""
    m = np.zeros((h, w), bool)
    for k in range(min(w, h)):
        m[h - 1 - k, k] = True
        m[h - 1 - k, w - 1 - k] = True
    return m
