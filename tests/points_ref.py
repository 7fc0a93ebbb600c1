"""ctypes front of tests/points_reference.cc, the serial CPU restatement of
the point export: compiled once per session with
g++ -O2 -ffp-contract=off into a temporary directory."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None

VERTEX_CLASS = {"unref": 0, "simple": 1, "border": 2, "complex": 3}
# `Variant` of points_reference.cc: 0 is the pinned behaviour, every other value
# gets one rule wrong (what test_export_cases_cpu.py counts)
VARIANTS = {None: 0, "P2_tie_le": 1, "P3_ge": 2, "P3_footprint_max": 3, "P3_no_sqrt2": 4,
            "P8_prepend_first": 5, "P9_unsorted": 6, "P10_complex_seeds": 7,
            "S6_latest": 8, "S7_ge": 9, "S8_multiply": 10, "S10_ge4": 11,
            "S10_own_triangle": 12, "S3_no_fallback": 13}
# the counters of points_ref_view's stats
STAT_MASK, STAT_TIES, STAT_EDGES, STAT_DISC, STAT_AXIS, STAT_DIAG, STAT_EQUAL, STAT_COUNT = (
    0, 16, 17, 18, 19, 22, 25, 26)


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="points_ref_"), "libpoints_ref.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC",
                               "-shared", "-o", out, os.path.join(HERE, "points_reference.cc")])
        _lib = C.CDLL(out)
        _lib.points_ref_view.restype = C.c_int64
        _lib.points_ref_footprint.restype = C.c_float
    return _lib


def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def footprint(w, h, flen, x, y, d):
    """P4: pixel_footprint of pixel (x, y) at depth d in a w x h view."""
    return np.float32(lib().points_ref_footprint(w, h, C.c_float(flen), x, y, C.c_float(d)))


def view(cam, dm, wnormals, image, dd_factor=5.0, variant=None):
    """One view: dm (h, w) ray-length depth to triangulate, wnormals (h, w, 3)
    world space, image (h, w[, c]) uint8 -> dict of numpy arrays (stats: the
    counters STAT_* of what the triangulation met)."""
    dm = np.ascontiguousarray(dm, np.float32)
    h, w = dm.shape
    wn = np.ascontiguousarray(wnormals, np.float32).reshape(h, w, 3)
    im = np.ascontiguousarray(image, np.uint8)
    ch = 1 if im.ndim == 2 else im.shape[2]
    rot = np.ascontiguousarray(np.asarray(cam.R, np.float32).reshape(9))
    trans = np.ascontiguousarray(np.asarray(cam.t, np.float32).reshape(3))
    n = w * h
    xyz = np.zeros((n, 3), np.float32)
    nrm = np.zeros((n, 3), np.float32)
    rgb = np.zeros((n, 3), np.uint8)
    conf = np.zeros(n, np.float32)
    val = np.zeros(n, np.float32)
    faces = np.zeros((max(2 * n, 1), 3), np.uint32)
    vclass = np.zeros(n, np.int32)
    nf = C.c_int64(0)
    stats = np.zeros(STAT_COUNT, np.int64)
    k = lib().points_ref_view(w, h, C.c_float(cam.flen), _ptr(rot, C.c_float),
                              _ptr(trans, C.c_float), _ptr(dm, C.c_float),
                              _ptr(wn, C.c_float), _ptr(im, C.c_uint8), ch,
                              C.c_float(dd_factor), _ptr(xyz, C.c_float),
                              _ptr(nrm, C.c_float), _ptr(rgb, C.c_uint8),
                              _ptr(conf, C.c_float), _ptr(val, C.c_float),
                              _ptr(faces, C.c_uint32), C.byref(nf),
                              _ptr(vclass, C.c_int32), VARIANTS[variant],
                              _ptr(stats, C.c_int64))
    return {"xyz": xyz[:k], "normals": nrm[:k], "rgb": rgb[:k], "confidence": conf[:k],
            "value": val[:k], "faces": faces[:nf.value], "vclass": vclass[:k], "stats": stats}


def points(cams, dms, wnormals, images, aabb=None, dd_factor=5.0, variant=None):
    """All views merged in view-list order (face ids offset), then the AABB
    clip of app/smvsrecon.cc:306-319 (faces dropped when clipping)."""
    parts = [view(c, d, n, i, dd_factor, variant)
             for c, d, n, i in zip(cams, dms, wnormals, images)]
    out = {"stats": sum(p["stats"] for p in parts)}
    for key in ("xyz", "normals", "rgb", "confidence", "value", "vclass"):
        out[key] = np.concatenate([p[key] for p in parts])
    base = np.cumsum([0] + [len(p["xyz"]) for p in parts[:-1]])
    out["faces"] = np.concatenate([p["faces"] + np.uint32(b) for p, b in zip(parts, base)])
    if aabb is not None:
        lo = np.asarray(aabb[0], np.float32)
        hi = np.asarray(aabb[1], np.float32)
        keep = ~((out["xyz"] < lo) | (out["xyz"] > hi)).any(axis=1)
        out = {k: v[keep] for k, v in out.items() if k not in ("faces", "stats")}
    return out


def read_ply(path):
    """A small binary little-endian PLY reader: parses the header on its own
    and returns {property name: array} of the vertex element and the face
    count."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    assert lines[0] == "ply"
    assert lines[1] == "format binary_little_endian 1.0"
    types = {"float": "<f4", "uchar": "u1", "int": "<i4", "uint": "<u4"}
    elements = []
    for ln in lines[2:]:
        tok = ln.split()
        if not tok or tok[0] in ("comment", "end_header"):
            continue
        if tok[0] == "element":
            elements.append((tok[1], int(tok[2]), []))
        elif tok[0] == "property":
            elements[-1][2].append(tuple(tok[1:]))
    name, count, props = elements[0]
    assert name == "vertex"
    dtype = np.dtype([(p[1], types[p[0]]) for p in props])
    vert = np.frombuffer(data, dtype=dtype, count=count, offset=end)
    faces = [e for e in elements[1:] if e[0] == "face"]
    return {k: vert[k].copy() for k in dtype.names}, [p[1] for p in props], \
        (faces[0][1] if faces else None), len(data) - end - count * dtype.itemsize
