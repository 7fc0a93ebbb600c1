#!/usr/bin/env python3
"""Times the mesh clean (smvs_mesh_clean) on fused
meshes of tools/tsdf_bench.py's scene (16 views of 960 x 540 around the
synthetic sphere's front, the cut on): 256^3 dense, 512^3 and 1024^3 sparse.
Per size: the fused mesh; clean_mesh box to box (upload, the kernels, download
of the result); the kernels alone, from the kernel trace of a child process
that runs the entry under rocprofv3 (--no-kernels skips it); the bytes the
clean has to move (every input array read once, every output array written
once) over the kernels' time and the fraction of the HBM copy rate
tools/peaks.py measures on the same GPU (--no-peaks: left out); and the time of
the same partition on the host's CPU (scipy.sparse.csgraph where it imports,
else the numpy restatement tests/mesh_clean_ref.py).  One JSON line each.

    python tools/mesh_clean_bench.py [--sizes dense:256 sparse:512 sparse:1024]
                                     [--percentile P] [--component-size N] [--reps N]
                                     [--no-kernels] [--no-peaks] [--no-cpu]

The synthetic scene's fusion has little junk: what is timed is the work of a
clean that keeps nearly everything, the evidence is synthetic, and the options
are untuned.
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

KERNELS = ["clean_init_kernel", "clean_select_hist_kernel", "clean_select_pick_kernel",
           "clean_vertex_flags_kernel", "clean_face_flags_kernel", "clean_union_kernel",
           "clean_count_kernel", "clean_apply_kernel", "scan_tile_sums_kernel",
           "scan_tiles_kernel", "scan_apply_kernel", "clean_compact_kernel",
           "clean_face_keep_kernel", "clean_face_compact_kernel", "clean_totals_kernel"]
MESH_KEYS = ("xyz", "normals", "rgb", "confidence", "faces")
CHILD_REPS = 3
VIEWS, SIZE = 16, (960, 540)


def fuse(kind, dims):
    from smvs_amd import device
    from points_bench import inputs
    from tsdf_bench import BOX_LO, BOX_SIDE
    cams, depths, normals, images = inputs(SIZE[0], SIZE[1], VIEWS)
    out = device.fuse_tsdf(cams, depths, normals, images, BOX_LO, BOX_SIDE / dims, (dims,) * 3,
                           cut=True, sparse=kind == "sparse")
    return {k: out[k] for k in MESH_KEYS + (("cells",) if kind == "sparse" else ())}


def options(args):
    return dict(percentile=args.percentile, component_size=args.component_size)


def child(args):
    from smvs_amd import device
    with np.load(args.child) as z:
        mesh = {k: z[k] for k in z.files}
    for _ in range(CHILD_REPS):
        device.clean_mesh(mesh, **options(args))


def kernel_times(args, mesh_file):
    """-> {kernel: (launches per call, best total seconds per call)}"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "-o", "run",
               "--", sys.executable, os.path.abspath(__file__), "--child", mesh_file,
               "--percentile", str(args.percentile), "--component-size",
               str(args.component_size)]
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if res.returncode != 0:
            raise RuntimeError("rocprofv3 failed: " + res.stderr[-2000:])
        files = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            raise RuntimeError("rocprofv3 left no kernel trace")
        rows = {k: [] for k in KERNELS}
        for fn in files:
            with open(fn) as f:
                for r in csv.DictReader(f):
                    for k in KERNELS:
                        if k in r["Kernel_Name"]:
                            rows[k].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    out = {}
    for k, v in rows.items():
        v.sort()
        if len(v) % CHILD_REPS:
            raise RuntimeError("%d launches of %s in the trace of %d calls"
                               % (len(v), k, CHILD_REPS))
        per = len(v) // CHILD_REPS
        if per:
            out[k] = (per, min(sum(1e-9 * (e - s) for s, e in v[i * per:(i + 1) * per])
                               for i in range(CHILD_REPS)))
    return out


def cpu_components(mesh, got):
    """the partition of the uncut vertices alone on the CPU -> (what ran, seconds)"""
    uncut = got["component"] != 0xFFFFFFFF
    f = mesh["faces"].astype(np.int64)
    f = f[uncut[f].all(1) & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])]
    n = uncut.size
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        import mesh_clean_ref
        t0 = time.perf_counter()
        mesh_clean_ref.components(n, f)
        return "tests/mesh_clean_ref.py components", time.perf_counter() - t0
    t0 = time.perf_counter()
    a = np.concatenate([f[:, 0], f[:, 1]])
    b = np.concatenate([f[:, 1], f[:, 2]])
    count, _lab = connected_components(coo_matrix((np.ones(a.size, np.int8), (a, b)),
                                                  shape=(n, n)), directed=False)
    dt = time.perf_counter() - t0
    assert count - int((~uncut).sum()) == got["stats"]["n_components"]
    return "scipy.sparse.csgraph.connected_components", dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", help=argparse.SUPPRESS)
    ap.add_argument("--sizes", nargs="+", default=["dense:256", "sparse:512", "sparse:1024"])
    ap.add_argument("--percentile", type=float, default=10.0)
    ap.add_argument("--component-size", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--no-peaks", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    if args.child:
        child(args)
        return
    import smvs_amd
    from smvs_amd import device
    if smvs_amd.device_count() < 1:
        raise SystemExit("mesh_clean_bench needs a GPU")
    copy_peak = None
    if not args.no_peaks:
        import peaks
        copy_peak = peaks.run()["hbm_copy_GBps"]
    for size in args.sizes:
        kind, dims = size.split(":")
        dims = int(dims)
        mesh = fuse(kind, dims)
        n, m = len(mesh["xyz"]), len(mesh["faces"])
        times = []
        for _ in range(args.reps + 1):
            t0 = time.perf_counter()
            got = device.clean_mesh(mesh, labels=True, **options(args))
            times.append(time.perf_counter() - t0)
        n2, m2 = len(got["xyz"]), len(got["faces"])
        per_vertex = 31 + (8 if kind == "sparse" else 0)
        moved = per_vertex * (n + n2) + 12 * (m + m2)
        entry = {"case": "entry", "fusion": kind, "dims": [dims] * 3, "vertices": n, "faces": m,
                 "vertices_out": n2, "faces_out": m2, "options": options(args),
                 "clean_ms_first": round(1e3 * times[0], 2),
                 "clean_ms_best": round(1e3 * min(times[1:]), 2),
                 "bytes_moved_MB": round(1e-6 * moved, 2)}
        entry.update(got["stats"])
        print(json.dumps(entry), flush=True)
        if not args.no_cpu:
            what, dt = cpu_components(mesh, got)
            print(json.dumps({"case": "cpu_components", "dims": [dims] * 3, "what": what,
                              "ms": round(1e3 * dt, 2)}), flush=True)
        if args.no_kernels:
            continue
        with tempfile.TemporaryDirectory() as tmp:
            mesh_file = os.path.join(tmp, "mesh.npz")
            np.savez(mesh_file, **mesh)
            kt = kernel_times(args, mesh_file)
        total = sum(t for _, t in kt.values())
        for k in KERNELS:
            if k in kt:
                per, t = kt[k]
                print(json.dumps({"case": "kernel", "dims": [dims] * 3, "kernel": k,
                                  "launches_per_call": per,
                                  "ms_per_call_best": round(1e3 * t, 4),
                                  "share": round(t / total, 3)}), flush=True)
        rec = {"case": "kernels_total", "dims": [dims] * 3,
               "ms_per_call_best": round(1e3 * total, 3),
               "bytes_moved_MB": round(1e-6 * moved, 2), "GBps": round(1e-9 * moved / total, 1)}
        if copy_peak:
            rec["hbm_copy_peak_GBps"] = round(copy_peak, 1)
            rec["fraction_of_hbm_copy_peak"] = round(1e-9 * moved / total / copy_peak, 4)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
