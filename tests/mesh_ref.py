"""ctypes front of tests/mesh_reference.cc, the serial CPU restatement of the
triangle mesh export: compiled once per session with
g++ -O2 -ffp-contract=off into a temporary directory.  Its input is the merged
mesh of tests/points_ref.py (M1)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import points_ref  # tests/points_ref.py

HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="mesh_ref_"), "libmesh_ref.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC",
                               "-shared", "-o", out, os.path.join(HERE, "mesh_reference.cc")])
        _lib = C.CDLL(out)
        _lib.mesh_ref_run.restype = C.c_int64
    return _lib


def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def finish(xyz, rgb, confidence, faces, aabb=None):
    """M2 (with smvsrecon's AABB list when aabb is (min3, max3)) and M3-M5 on a
    merged mesh -> dict xyz, normals, rgb, confidence, faces."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    rgb = np.ascontiguousarray(rgb, np.uint8).reshape(n, 3)
    conf = np.ascontiguousarray(confidence, np.float32).reshape(n)
    faces = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3)
    m = len(faces)
    lo = np.ascontiguousarray(aabb[0] if aabb is not None else np.zeros(3), np.float32)
    hi = np.ascontiguousarray(aabb[1] if aabb is not None else np.zeros(3), np.float32)
    out = {"xyz": np.zeros((n, 3), np.float32), "normals": np.zeros((n, 3), np.float32),
           "rgb": np.zeros((n, 3), np.uint8), "confidence": np.zeros(n, np.float32),
           "faces": np.zeros((max(m, 1), 3), np.uint32)}
    m_out = C.c_int64(0)
    k = lib().mesh_ref_run(C.c_int64(n), _ptr(xyz, C.c_float), _ptr(rgb, C.c_uint8),
                           _ptr(conf, C.c_float), C.c_int64(m), _ptr(faces, C.c_uint32),
                           int(aabb is not None), _ptr(lo, C.c_float), _ptr(hi, C.c_float),
                           _ptr(out["xyz"], C.c_float), _ptr(out["normals"], C.c_float),
                           _ptr(out["rgb"], C.c_uint8), _ptr(out["confidence"], C.c_float),
                           _ptr(out["faces"], C.c_uint32), C.byref(m_out))
    for key in ("xyz", "normals", "rgb", "confidence"):
        out[key] = out[key][:k]
    out["faces"] = out["faces"][:m_out.value]
    return out


def face_terms(xyz, faces):
    """M3 / M4 per face -> (fn (m, 3), weights (m, 3), counts (m,) bool)."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3)
    m = len(faces)
    fn = np.zeros((m, 3), np.float32)
    w = np.zeros((m, 3), np.float32)
    ok = np.zeros(m, np.int32)
    lib().mesh_ref_face_terms(C.c_int64(len(xyz)), _ptr(xyz, C.c_float), C.c_int64(m),
                              _ptr(faces, C.c_uint32), _ptr(fn, C.c_float),
                              _ptr(w, C.c_float), _ptr(ok, C.c_int32))
    return fn, w, ok.astype(bool)


def mesh(cams, dms, wnormals, images, aabb=None, dd_factor=5.0, variant=None):
    """smvsrecon --mesh: the views triangulated and merged by points_ref (M1:
    no values, no looked-up normals), then M2-M5."""
    merged = points_ref.points(cams, dms, wnormals, images, aabb=None, dd_factor=dd_factor,
                               variant=variant)
    return finish(merged["xyz"], merged["rgb"], merged["confidence"], merged["faces"], aabb)


def save_ply(path, m):
    """M6: the restatement's writer of a mesh dict."""
    xyz = np.ascontiguousarray(m["xyz"], np.float32)
    nrm = np.ascontiguousarray(m["normals"], np.float32)
    rgb = np.ascontiguousarray(m["rgb"], np.uint8)
    conf = np.ascontiguousarray(m["confidence"], np.float32)
    faces = np.ascontiguousarray(m["faces"], np.uint32)
    rc = lib().mesh_ref_save_ply(path.encode(), C.c_int64(len(conf)), _ptr(xyz, C.c_float),
                                 _ptr(nrm, C.c_float), _ptr(rgb, C.c_uint8),
                                 _ptr(conf, C.c_float), C.c_int64(len(faces)),
                                 _ptr(faces, C.c_uint32))
    if rc != 0:
        raise OSError("mesh_ref_save_ply: cannot write " + path)


def read_ply_mesh(path):
    """A binary little-endian PLY reader for vertex + face elements, written
    for these tests: -> (header lines, {property: array}, faces (m, 3) int32).
    Every face record must be a list of 3."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").rstrip("\n").split("\n")
    types = {"float": "<f4", "uchar": "u1", "int": "<i4", "uint": "<u4"}
    elements = []
    for ln in lines:
        tok = ln.split()
        if tok[0] == "element":
            elements.append((tok[1], int(tok[2]), []))
        elif tok[0] == "property":
            elements[-1][2].append(tok[1:])
    assert [e[0] for e in elements] == ["vertex", "face"]
    _, n, props = elements[0]
    dtype = np.dtype([(p[1], types[p[0]]) for p in props])
    vert = np.frombuffer(data, dtype=dtype, count=n, offset=end)
    _, m, fprops = elements[1]
    assert fprops == [["list", "uchar", "int", "vertex_indices"]]
    at = end + n * dtype.itemsize
    rec = np.dtype([("count", "u1"), ("ids", "<i4", (3,))])
    assert len(data) - at == m * rec.itemsize, "trailing or missing bytes"
    fr = np.frombuffer(data, dtype=rec, count=m, offset=at)
    assert np.all(fr["count"] == 3)
    return lines, {k: vert[k].copy() for k in dtype.names}, fr["ids"].copy()
