#!/usr/bin/env python3
"""Node initialisation at 1920 x 1080, init scales 4, 5 and 6, with and without a
slant plane: run under rocprofv3 --kernel-trace --stats to compare
surf_init_nodes_planes_kernel (csrc/surface_planes.hip) with the reference's
surf_init_nodes_kernel (csrc/surface.hip) in one session, and to time
surf_slant_tap_kernel (a 960 x 540 map).

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o run -- \\
        python tools/surface_planes_cost.py
    python tools/surface_planes_cost.py --summarise <dir>

One create per kernel launch; the three scales run different template instances
(4, 16 and 64 window pixels per lane), which the statistics keep apart by name."""
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

W, H, REPS = 1920, 1080, 10


def workload():
    import smvs_amd
    rng = np.random.default_rng(1)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    depth = (4.0 + 0.0005 * xx + 0.0003 * yy + 0.01 * rng.standard_normal((H, W))
             ).astype(np.float32)
    depth[rng.random((H, W)) < 0.05] = 0.0
    low = depth[::2, ::2].copy()
    g = (0.001 + 0.0005 * rng.standard_normal(low.shape + (2,))).astype(np.float32)
    g[rng.random(low.shape) < 0.1] = np.nan
    img = rng.integers(0, 256, size=(H, W, 3)).astype(np.uint8)
    ctx = smvs_amd.ViewContext(W, H, 1)
    ctx.upload_image(-1, img)
    ctx.sgm_init_depth(low)
    plane = None
    for _ in range(REPS):
        plane = ctx.sgm_init_slants(g)
    for scale in (4, 5, 6):
        for _ in range(REPS):
            a = ctx.create_surface(scale, depth=depth)
            b = ctx.create_surface(scale, depth=depth, slant=plane)
        assert np.array_equal(a["node_valid"], b["node_valid"])
        print("scale %d: %d nodes, %d valid patches" % (scale, a["node_valid"].size,
                                                       b["valid_patches"]))
    ctx.close()


def summarise(root):
    import csv
    path = glob.glob(os.path.join(root, "**", "*kernel_stats.csv"), recursive=True)[0]
    rows = [r for r in csv.DictReader(open(path))
            if "surf_init_nodes" in r["Name"] or "surf_slant_tap" in r["Name"]]
    print("%-78s %6s %12s %10s %10s" % ("kernel", "calls", "average us", "min us", "max us"))
    for r in sorted(rows, key=lambda r: r["Name"]):
        name = r["Name"].replace("smvs_hip::", "").split("(")[0]
        print("%-78s %6s %12.1f %10.1f %10.1f" % (name[:78], r["Calls"],
              float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--summarise":
        summarise(sys.argv[2])
    else:
        workload()
