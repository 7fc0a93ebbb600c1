#!/usr/bin/env python3
"""Times the triangle mesh export (smvs_mesh_generate, smvsrecon --mesh) at
1920x1080 for 9 and 64 views with the cut on; the download from the handle
and the PLY write on the host (save_ply_mesh) separately.  Prints one JSON
line per case.  Use under rocprofv3 --kernel-trace --stats for the
per-kernel split.  The inputs are tools/points_bench.py's (the 64-view input
repeats the nine synthetic views).

MESH_BENCH_VIEWS (default "9,64") and MESH_BENCH_REPS (default 3) pick the
cases; MESH_BENCH_AABB=1 adds a run per view count clipped to the box between
the 25th and 75th percentiles of the unclipped vertices (per axis), which cuts
faces in every view.  The PLY write is skipped (ply_write_ms null) when the
temporary directory has less free space than twice the file."""
import ctypes as C
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402

import smvs_amd  # noqa: E402
from smvs_amd import _capi, host  # noqa: E402
from smvs_amd.device import MeshOptions, _point_views, _fp, _u8p, _u32p, _p  # noqa: E402
from points_bench import inputs  # noqa: E402


def generate(cams, depths, normals, images, cut, reps, aabb=None):
    lib = _capi.load()
    arr, _, _keep = _point_views(cams, depths, normals, images, False)
    opt = MeshOptions(cut_surfaces=int(cut), dd_factor=5.0)
    if aabb is not None:
        opt.use_aabb = 1
        for k in range(3):
            opt.aabb_min[k], opt.aabb_max[k] = float(aabb[0][k]), float(aabb[1][k])
    times = []
    for r in range(reps):
        handle, nv, nf = C.c_void_p(), C.c_int64(), C.c_int64()
        t0 = time.perf_counter()
        _capi.check(lib.smvs_mesh_generate(0, arr, len(cams), C.byref(opt), C.byref(handle),
                                           C.byref(nv), C.byref(nf)))
        times.append(time.perf_counter() - t0)
        if r + 1 < reps:
            lib.smvs_points_release(handle)
    k, m = nv.value, nf.value
    out = {"xyz": np.empty((k, 3), np.float32), "normals": np.empty((k, 3), np.float32),
           "rgb": np.empty((k, 3), np.uint8), "confidence": np.empty(k, np.float32),
           "faces": np.empty((m, 3), np.uint32)}
    t0 = time.perf_counter()
    _capi.check(lib.smvs_points_download(handle, _p(out["xyz"], _fp), _p(out["normals"], _fp),
                                         _p(out["rgb"], _u8p), _p(out["confidence"], _fp),
                                         None, _p(out["faces"], _u32p)))
    t_dl = time.perf_counter() - t0
    lib.smvs_points_release(handle)
    return times, t_dl, out


def main():
    w, h = 1920, 1080
    views = [int(x) for x in os.environ.get("MESH_BENCH_VIEWS", "9,64").split(",")]
    reps = int(os.environ.get("MESH_BENCH_REPS", "3"))
    if smvs_amd.device_count() < 1:
        raise SystemExit("mesh_bench needs a GPU")
    for nv in views:
        cams, depths, normals, images = inputs(w, h, nv)
        aabbs = [None]
        while aabbs:
            aabb = aabbs.pop(0)
            times, t_dl, out = generate(cams, depths, normals, images, True, reps, aabb)
            n, m = len(out["xyz"]), len(out["faces"])
            ply_bytes = 31 * n + 13 * m
            t_ply = None
            with tempfile.TemporaryDirectory() as tmp:
                if shutil.disk_usage(tmp).free > 2 * ply_bytes:
                    t0 = time.perf_counter()
                    host.save_ply_mesh(os.path.join(tmp, "m.ply"), out["xyz"],
                                       out["normals"], out["rgb"], out["confidence"],
                                       out["faces"])
                    t_ply = time.perf_counter() - t0
            rec = {"views": nv, "size": [w, h], "cut": True,
                   "aabb": None if aabb is None else [list(map(float, x)) for x in aabb],
                   "vertices": n, "faces": m,
                   "generate_ms_first": round(1e3 * times[0], 2),
                   "generate_ms_best": round(1e3 * min(times), 2),
                   "download_ms": round(1e3 * t_dl, 2),
                   "ply_write_ms": None if t_ply is None else round(1e3 * t_ply, 2),
                   "ply_bytes": ply_bytes}
            print(json.dumps(rec), flush=True)
            if aabb is None and os.environ.get("MESH_BENCH_AABB") == "1":
                q = np.percentile(out["xyz"], [25, 75], axis=0).astype(np.float32)
                aabbs.append((q[0], q[1]))
            del out


if __name__ == "__main__":
    main()
