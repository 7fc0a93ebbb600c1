#!/usr/bin/env python3
"""Times smvsrecon --simplify on the device (smvs_simplified_generate,
DESIGN.md section 9.7): per call and per view at 480x270 and 1920x1080 for 9
and 64 views (cut on, point cloud), the split of one view's persistent
workgroup into selection / Delaunay lane / rescans from the stamped build of
the kernel (smvs_simplify_triangulate with clocks), and the serial CPU
restatement (tests/simplify_reference.cc, one core of the same machine) on the
same map, with an array_equal check of the two triangulations.  Prints one
JSON line per case.  Use under rocprofv3 --kernel-trace --stats for the
per-kernel times.  The inputs are tools/points_bench.py's with 0.2 % noise.

SIMPLIFY_BENCH_SIZES (default "480x270,1920x1080"), SIMPLIFY_BENCH_VIEWS
(default "9,64") and SIMPLIFY_BENCH_REPS (default 2) pick the cases."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import smvs_amd  # noqa: E402
import simplify_ref  # noqa: E402  (tests/simplify_ref.py)
from points_bench import inputs  # noqa: E402


def noisy(depths, seed=2):
    rng = np.random.default_rng(seed)
    return [np.ascontiguousarray(d * (1.0 + 0.002 * rng.standard_normal(d.shape)), np.float32)
            for d in depths]


def main():
    if smvs_amd.device_count() < 1:
        raise SystemExit("simplify_bench needs a GPU")
    sizes = [tuple(int(v) for v in s.split("x"))
             for s in os.environ.get("SIMPLIFY_BENCH_SIZES", "480x270,1920x1080").split(",")]
    views = [int(x) for x in os.environ.get("SIMPLIFY_BENCH_VIEWS", "9,64").split(",")]
    reps = int(os.environ.get("SIMPLIFY_BENCH_REPS", "2"))
    simplify_ref.lib()   # (compiles the restatement: not part of its time)
    for w, h in sizes:
        cams, depths, normals, images = inputs(w, h, 9)
        depths = noisy(depths)
        # one view: the device against the restatement, and the kernel's split
        t0 = time.perf_counter()
        want = simplify_ref.triangulate(depths[0])
        t_ref = time.perf_counter() - t0
        best, got = None, None
        for _ in range(reps):
            t0 = time.perf_counter()
            got = smvs_amd.simplify_triangulate(depths[0])
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        same = (got["iterations"] == want["iterations"]
                and np.array_equal(got["vertices"], want["vertices"])
                and np.array_equal(got["triangles"], want["triangles"])
                and np.array_equal(got["num_zero_depths"], want["num_zero_depths"]))
        ticks = smvs_amd.simplify_triangulate(depths[0], clocks=True)["clocks"].astype(float)
        print(json.dumps({"case": "one view", "size": [w, h],
                          "iterations": got["iterations"], "array_equal": bool(same),
                          "device_call_ms": round(1e3 * best, 2),
                          "restatement_one_core_ms": round(1e3 * t_ref, 2),
                          "stamped_kernel_ms": round(ticks[3] / 1e5, 2),
                          "share_selection": round(ticks[0] / ticks[3], 3),
                          "share_delaunay_lane": round(ticks[1] / ticks[3], 3),
                          "share_rescans": round(ticks[2] / ticks[3], 3)}), flush=True)
        if not same:
            raise SystemExit("device and restatement differ at %dx%d" % (w, h))
        for nv in views:
            pick = [i % 9 for i in range(nv)]
            args = ([cams[i] for i in pick], [depths[i] for i in pick],
                    [normals[i] for i in pick], [images[i] for i in pick])
            times = []
            for _ in range(reps):
                t0 = time.perf_counter()
                out = smvs_amd.generate_simplified(*args)
                times.append(time.perf_counter() - t0)
            print(json.dumps({"case": "generate_simplified", "size": [w, h], "views": nv,
                              "vertices": len(out["xyz"]), "faces": len(out["faces"]),
                              "call_ms_first": round(1e3 * times[0], 2),
                              "call_ms_best": round(1e3 * min(times), 2),
                              "per_view_ms": round(1e3 * min(times) / nv, 2)}), flush=True)


if __name__ == "__main__":
    main()
