#!/usr/bin/env python3
"""Times the point export (smvs_points_generate) at 1920x1080 for 9 and 64
views, cut on and off; the download from the handle and the PLY write on
the host separately; and the serial CPU restatement (tests/points_reference.cc)
on the 9-view input without the cut.  Prints one JSON line per case.  Use
under rocprofv3 --kernel-trace --stats for the per-kernel split.

The 64-view input repeats the nine synthetic views (sphere in front of a
plane, synth.ring_cameras) cyclically."""
import ctypes as C
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import smvs_amd  # noqa: E402
from smvs_amd import _capi, host, synth  # noqa: E402
from smvs_amd.device import PointView, PointsOptions, _fp, _u8p, _p  # noqa: E402


def inputs(w, h, n_views):
    main, subs = synth.ring_cameras(w, h, 8)
    cams9 = [main] + subs
    scene = synth.SphereScene(px_size=3.0 / (1.2 * w))
    d9, n9 = synth.depth_and_normal_maps(scene, cams9)
    rng = np.random.default_rng(1)
    im9 = [rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for _ in cams9]
    pick = [i % 9 for i in range(n_views)]
    return ([cams9[i] for i in pick], [d9[i] for i in pick], [n9[i] for i in pick],
            [im9[i] for i in pick])


def generate(cams, depths, normals, images, cut, reps):
    lib = _capi.load()
    n = len(cams)
    arr = (PointView * n)()
    for i in range(n):
        h, w = depths[i].shape
        arr[i].width, arr[i].height, arr[i].flen = w, h, float(cams[i].flen)
        for k, x in enumerate(np.asarray(cams[i].R, np.float32).reshape(9)):
            arr[i].rot[k] = float(x)
        for k, x in enumerate(np.asarray(cams[i].t, np.float32).reshape(3)):
            arr[i].trans[k] = float(x)
        arr[i].depth = _p(depths[i], _fp)
        arr[i].normals = _p(normals[i], _fp)
        arr[i].image = _p(images[i], _u8p)
        arr[i].channels = 3
    opt = PointsOptions(cut_surfaces=int(cut), dd_factor=5.0)
    times = []
    for _ in range(reps):
        handle, npts = C.c_void_p(), C.c_int64()
        t0 = time.perf_counter()
        _capi.check(lib.smvs_points_generate(0, arr, n, C.byref(opt), C.byref(handle),
                                             C.byref(npts)))
        times.append(time.perf_counter() - t0)
        if _ + 1 < reps:
            lib.smvs_points_release(handle)
    k = npts.value
    out = {"xyz": np.empty((k, 3), np.float32), "normals": np.empty((k, 3), np.float32),
           "rgb": np.empty((k, 3), np.uint8), "confidence": np.empty(k, np.float32),
           "value": np.empty(k, np.float32)}
    t0 = time.perf_counter()
    _capi.check(lib.smvs_points_download(handle, _p(out["xyz"], _fp), _p(out["normals"], _fp),
                                         _p(out["rgb"], _u8p), _p(out["confidence"], _fp),
                                         _p(out["value"], _fp), None))
    t_dl = time.perf_counter() - t0
    lib.smvs_points_release(handle)
    return times, t_dl, out


def main():
    w, h = 1920, 1080
    views = [int(x) for x in os.environ.get("POINTS_BENCH_VIEWS", "9,64").split(",")]
    reps = int(os.environ.get("POINTS_BENCH_REPS", "3"))
    if smvs_amd.device_count() < 1:
        raise SystemExit("points_bench needs a GPU")
    for nv in views:
        cams, depths, normals, images = inputs(w, h, nv)
        for cut in (True, False):
            times, t_dl, out = generate(cams, depths, normals, images, cut, reps)
            with tempfile.TemporaryDirectory() as tmp:
                t0 = time.perf_counter()
                host.save_ply_points(os.path.join(tmp, "p.ply"), out["xyz"], out["normals"],
                                     out["rgb"], out["confidence"], out["value"])
                t_ply = time.perf_counter() - t0
            rec = {"views": nv, "size": [w, h], "cut": cut, "points": len(out["xyz"]),
                   "generate_ms_first": round(1e3 * times[0], 2),
                   "generate_ms_best": round(1e3 * min(times), 2),
                   "download_ms": round(1e3 * t_dl, 2), "ply_write_ms": round(1e3 * t_ply, 2)}
            if nv == 9 and not cut and "--no-cpu" not in sys.argv:
                import points_ref
                from oracle import pyoracle
                wn = []
                for c, d, n in zip(cams, depths, normals):
                    wn.append(pyoracle.cut_depth_maps([c], [d], [n])[1][0])
                t0 = time.perf_counter()
                ref = points_ref.points(cams, depths, wn, images)
                rec["cpu_restatement_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
                rec["cpu_equal"] = all(np.array_equal(ref[k], out[k]) for k in
                                       ("xyz", "normals", "rgb", "confidence", "value"))
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
