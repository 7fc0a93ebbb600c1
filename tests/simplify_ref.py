"""ctypes front of tests/simplify_reference.cc, the serial CPU restatement of
smvsrecon --simplify: compiled once per session with
g++ -O2 -ffp-contract=off into a temporary directory.  The merge (M1), the
AABB clip (M2) and recalc_normals (M3-M5) are those of tests/mesh_ref.py."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import mesh_ref  # tests/mesh_ref.py
from points_ref import VARIANTS  # tests/points_ref.py

HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="simplify_ref_"), "libsimplify_ref.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC",
                               "-shared", "-o", out,
                               os.path.join(HERE, "simplify_reference.cc")])
        _lib = C.CDLL(out)
        for name in ("simplify_ref_triangulate", "simplify_ref_view", "simplify_ref_pixels",
                     "simplify_ref_delaunay", "simplify_ref_delete_invalid_faces"):
            getattr(_lib, name).restype = C.c_int64
    return _lib


# the counters of simplify_ref_view's and simplify_ref_triangulate's stats
(SSTAT_ZERO, SSTAT_RATIO, SSTAT_FOUR, SSTAT_FIVE, SSTAT_OTHER, SSTAT_NEAR, SSTAT_TIED_TOPS,
 SSTAT_TIED_SCANS, SSTAT_NOOP, SSTAT_ROWS, SSTAT_ITERATIONS, SSTAT_VALID, SSTAT_COUNT) = range(13)


def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def budget(w, h, max_vertices=-1):
    """S1: the number of loop iterations allowed."""
    return (w * h) // 40 if max_vertices < 0 else int(max_vertices)


def triangulate(dm, max_vertices=-1, max_error=-1.0, variant=None):
    """S1-S8 on one depth map -> dict iterations, vertices (n, 3) float64,
    triangles (t, 3) uint32, num_zero_depths (t,) int32, stats (the counters
    SSTAT_* of what the loop met)."""
    dm = np.ascontiguousarray(dm, np.float32)
    h, w = dm.shape
    b = budget(w, h, max_vertices)
    verts = np.zeros((b + 4, 3), np.float64)
    tris = np.zeros((2 * b + 2, 3), np.uint32)
    nzero = np.zeros(2 * b + 2, np.int32)
    nv, nt = C.c_int64(0), C.c_int64(0)
    stats = np.zeros(SSTAT_COUNT, np.int64)
    with np.errstate(all="ignore"):
        it = lib().simplify_ref_triangulate(w, h, _ptr(dm, C.c_float), int(max_vertices),
                                            C.c_double(max_error), _ptr(verts, C.c_double),
                                            C.byref(nv), _ptr(tris, C.c_uint32),
                                            _ptr(nzero, C.c_int32), C.byref(nt),
                                            VARIANTS[variant], _ptr(stats, C.c_int64))
    return {"iterations": int(it), "vertices": verts[:nv.value], "triangles": tris[:nt.value],
            "num_zero_depths": nzero[:nt.value], "stats": stats}


def view(cam, dm, wnormals, image, max_vertices=-1, max_error=-1.0, variant=None):
    """One view of generate_mesh with Options::simplify -> dict of arrays."""
    dm = np.ascontiguousarray(dm, np.float32)
    h, w = dm.shape
    wn = np.ascontiguousarray(wnormals, np.float32).reshape(h, w, 3)
    im = np.ascontiguousarray(image, np.uint8)
    ch = 1 if im.ndim == 2 else im.shape[2]
    rot = np.ascontiguousarray(np.asarray(cam.R, np.float32).reshape(9))
    trans = np.ascontiguousarray(np.asarray(cam.t, np.float32).reshape(3))
    n = budget(w, h, max_vertices) + 4
    xyz = np.zeros((n, 3), np.float32)
    nrm = np.zeros((n, 3), np.float32)
    rgb = np.zeros((n, 3), np.uint8)
    conf = np.zeros(n, np.float32)
    val = np.zeros(n, np.float32)
    faces = np.zeros((2 * n, 3), np.uint32)
    nf = C.c_int64(0)
    stats = np.zeros(SSTAT_COUNT, np.int64)
    vclass = np.zeros(n, np.int32)
    k = lib().simplify_ref_view(w, h, C.c_float(cam.flen), _ptr(rot, C.c_float),
                                _ptr(trans, C.c_float), _ptr(dm, C.c_float),
                                _ptr(wn, C.c_float), _ptr(im, C.c_uint8), ch,
                                int(max_vertices), C.c_double(max_error),
                                _ptr(xyz, C.c_float), _ptr(nrm, C.c_float),
                                _ptr(rgb, C.c_uint8), _ptr(conf, C.c_float),
                                _ptr(val, C.c_float), _ptr(faces, C.c_uint32), C.byref(nf),
                                VARIANTS[variant], _ptr(stats, C.c_int64),
                                _ptr(vclass, C.c_int32))
    return {"xyz": xyz[:k], "normals": nrm[:k], "rgb": rgb[:k], "confidence": conf[:k],
            "value": val[:k], "faces": faces[:nf.value], "stats": stats, "vclass": vclass[:k]}


def simplified(cams, dms, wnormals, images, mesh=False, aabb=None, max_vertices=-1,
               max_error=-1.0, variant=None):
    """All views merged in view-list order (S13).  mesh=False: the point cloud
    (values, looked-up normals; the faces unless clipped); mesh=True: M2-M5."""
    parts = [view(c, d, n, i, max_vertices, max_error, variant)
             for c, d, n, i in zip(cams, dms, wnormals, images)]
    out = {"stats": sum(p["stats"] for p in parts)}
    out["stats"][SSTAT_ROWS] = max(p["stats"][SSTAT_ROWS] for p in parts)
    for key in ("xyz", "normals", "rgb", "confidence", "value", "vclass"):
        out[key] = np.concatenate([p[key] for p in parts])
    base = np.cumsum([0] + [len(p["xyz"]) for p in parts[:-1]])
    out["faces"] = np.concatenate([p["faces"] + np.uint32(b) for p, b in zip(parts, base)])
    if mesh:
        return mesh_ref.finish(out["xyz"], out["rgb"], out["confidence"], out["faces"], aabb)
    if aabb is not None:
        lo = np.asarray(aabb[0], np.float32)
        hi = np.asarray(aabb[1], np.float32)
        keep = ~((out["xyz"] < lo) | (out["xyz"] > hi)).any(axis=1)
        out = {k: v[keep] for k, v in out.items() if k not in ("faces", "stats")}
    return out


def pixels(a, b, c):
    """S8: the pixels of triangle (a, b, c) in emission order, (n, 2) int32."""
    abc = np.ascontiguousarray(np.asarray([a, b, c], np.float64).reshape(6))
    n = lib().simplify_ref_pixels(_ptr(abc, C.c_double), None, C.c_int64(0))
    xy = np.zeros((max(n, 1), 2), np.int32)
    lib().simplify_ref_pixels(_ptr(abc, C.c_double), _ptr(xy, C.c_int32), C.c_int64(n))
    return xy[:n]


def delaunay(points, lo, hi):
    """S4 / S5: points inserted one by one into the quad [lo, hi]^2 ->
    (vertices count, triangles (t, 3), changed-set size per insertion)."""
    pts = np.ascontiguousarray(points, np.float64).reshape(-1, 2)
    n = len(pts)
    tris = np.zeros((2 * n + 2, 3), np.uint32)
    changed = np.zeros(max(n, 1), np.int32)
    nv = C.c_int64(0)
    t = lib().simplify_ref_delaunay(C.c_double(lo), C.c_double(hi), C.c_int64(n),
                                    _ptr(pts, C.c_double), _ptr(tris, C.c_uint32),
                                    _ptr(changed, C.c_int32), C.byref(nv))
    return nv.value, tris[:t], changed[:n]


def heap_order(keys):
    """S6: ids in the order begin() hands them out after emplacing keys in order."""
    k = np.ascontiguousarray(keys, np.float64)
    order = np.zeros(len(k), np.int64)
    lib().simplify_ref_heap_order(C.c_int64(len(k)), _ptr(k, C.c_double), _ptr(order, C.c_int64))
    return order


def delete_invalid_faces(faces):
    """S11 on a face list (m, 3) -> the faces left, in the order it leaves them."""
    f = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3).copy()
    m = lib().simplify_ref_delete_invalid_faces(C.c_int64(len(f)), _ptr(f, C.c_uint32))
    return f[:m]
