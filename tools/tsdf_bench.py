#!/usr/bin/env python3
"""Times the volumetric fusion (smvs_tsdf_fuse) at 256^3 voxels with 16 views
of 960 x 540 around the synthetic sphere's front, the cut on: the entry box to
box (upload, preparation and cut, integration, extraction, download of the
mesh), and the kernels alone -- from the kernel trace of a child process that
runs the entry under rocprofv3 (--no-kernels skips it).  Prints one JSON line
for the entry and one per kernel; the integration kernel's line carries the
bytes it has to move (the volume written once, 24 bytes per voxel, and every
depth map read once) over its time, and the fraction of the HBM copy rate
tools/peaks.py measures on the same GPU (--no-peaks: left out).  The inputs are
tools/points_bench.py's (the 16 views repeat the nine synthetic ones).

    python tools/tsdf_bench.py [--dims N] [--views N] [--size W H] [--reps N]
                               [--no-kernels] [--no-peaks]
                               [--sparse [--resolution N] [--max-bricks N] [--cull]]
                               [--batch N [--no-cut]]
                               [--sparse --batch N [--no-cut] [--cull]]

--sparse times smvs_tsdf_fuse_sparse (the brick-sparse volume, DESIGN.md section
9.9) on the same case instead: --resolution N is --dims N and may go up to
4096.  The entry's line carries the stats (bricks, seed and allocated bricks,
state bytes, the dense volume's would-be bytes); the seed kernel's line its
time per 1000 (voxel, view) pairs of the whole box, the integration kernel's
its time per 1000 pairs of the allocated bricks.  --cull puts the brick cull
(section 9.10) in front of the seed pass: the entry's line gains tested_bricks,
their share and the pyramids' bytes, and the pyramid, cull, list and listed-seed
kernels take the seed kernel's place.

--batch N times the persistent volume (smvs_tsdf_volume, section 9.13) on the
same case against the one-shot entry in the same process: create, integrate
per batch of N views, extract, release -- box to box, the two entries
alternating -- and the kernels of both from one trace each.  With the cut on a
batch is cut within itself, which is less work than the one-shot's cut and
another mesh; --no-cut compares like with like (the meshes are then equal, and
the tool checks that they are).

--sparse --batch N times the persistent brick-sparse volume
(smvs_tsdf_sparse_volume, section 9.14) against the one-shot sparse entry in
the same way: create, mark per batch of N views (--cull: with the brick cull in
front), integrate per batch without growth, extract, release.  The entry's line
carries the time of the mark pass, of the integrate pass (the first integrate
gives every brick its slot) and of the extraction, and the volume's stats.
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
import numpy as np  # noqa: E402

KERNELS = ["mesh_prepare_kernel", "mesh_cut_kernel", "tsdf_depth_kernel", "tsdf_integrate_kernel",
           "tsdf_classify_kernel", "scan_tile_sums_kernel", "scan_tiles_kernel",
           "scan_apply_kernel", "tsdf_vertex_kernel", "tsdf_face_kernel"]
SPARSE_KERNELS = ["mesh_prepare_kernel", "mesh_cut_kernel", "tsdf_depth_kernel",
                  "tsdf_sparse_seed_kernel", "tsdf_sparse_dilate_kernel",
                  "tsdf_sparse_table_kernel", "tsdf_sparse_integrate_kernel",
                  "tsdf_sparse_classify_kernel", "scan_tile_sums_kernel", "scan_tiles_kernel",
                  "scan_apply_kernel", "tsdf_sparse_vertex_kernel", "tsdf_sparse_face_kernel"]
# with --cull: the pyramids, the cull and the seed pass over the candidate list
# in the place of tsdf_sparse_seed_kernel (the scan runs twice more)
CULL_KERNELS = ["tsdf_pyramid_tile_kernel", "tsdf_pyramid_top_kernel", "tsdf_cull_kernel",
                "tsdf_cull_list_kernel", "tsdf_sparse_seed_list_kernel"]
# with --batch: the preparation runs per batch, the integration on the stored sums
VOLUME_KERNELS = ["mesh_prepare_kernel", "mesh_cut_kernel", "tsdf_depth_kernel",
                  "tsdf_volume_integrate_kernel", "tsdf_volume_field_kernel",
                  "tsdf_classify_kernel", "scan_tile_sums_kernel", "scan_tiles_kernel",
                  "scan_apply_kernel", "tsdf_vertex_kernel", "tsdf_face_kernel"]
# with --sparse --batch: per batch the preparation twice (mark, integrate), the
# seed pass and its merge; the slots once; the integration on the stored sums
SPARSE_VOLUME_KERNELS = ["mesh_prepare_kernel", "mesh_cut_kernel", "tsdf_depth_kernel",
                         "tsdf_sparse_seed_kernel", "tsdf_sparse_volume_merge_kernel",
                         "tsdf_sparse_dilate_kernel", "tsdf_sparse_table_kernel",
                         "tsdf_sparse_volume_reslot_kernel",
                         "tsdf_sparse_volume_integrate_kernel",
                         "tsdf_sparse_volume_field_kernel", "tsdf_sparse_classify_kernel",
                         "scan_tile_sums_kernel", "scan_tiles_kernel", "scan_apply_kernel",
                         "tsdf_sparse_vertex_kernel", "tsdf_sparse_face_kernel"]
CHILD_REPS = 3
BOX_LO, BOX_SIDE = (-1.3, -1.3, 2.7), 2.6


def case(args):
    from points_bench import inputs
    cams, depths, normals, images = inputs(args.size[0], args.size[1], args.views)
    return cams, depths, normals, images, BOX_LO, BOX_SIDE / args.dims, (args.dims,) * 3


def sparse_args(args):
    if not args.sparse:
        return {}
    out = {"sparse": True, "max_bricks": args.max_bricks}
    if args.cull:
        out["cull"] = True
    return out


def sparse_kernels(args):
    if not args.cull:
        return SPARSE_KERNELS
    at = SPARSE_KERNELS.index("tsdf_sparse_seed_kernel")
    return SPARSE_KERNELS[:at] + CULL_KERNELS + SPARSE_KERNELS[at + 1:]


def fuse_batched(c, batch, cut):
    """create, integrate per batch of `batch` views, extract, release"""
    from smvs_amd import device
    cams, depths, normals, images, origin, voxel, dims = c
    with device.TsdfVolume(origin, voxel, dims) as vol:
        for at in range(0, len(cams), batch):
            vol.integrate(cams[at:at + batch], depths[at:at + batch], normals[at:at + batch],
                          images[at:at + batch], cut=cut)
        return vol.extract()


def fuse_sparse_batched(c, args, times=None):
    """create, mark per batch, integrate per batch without growth, extract,
    release; times (a dict): the seconds of the three passes are added to it"""
    from smvs_amd import device
    cams, depths, normals, images, origin, voxel, dims = c
    cut, n = not args.no_cut, args.batch
    with device.SparseTsdfVolume(origin, voxel, dims, max_bricks=args.max_bricks) as vol:
        t0 = time.perf_counter()
        for at in range(0, len(cams), n):
            vol.mark(cams[at:at + n], depths[at:at + n], normals[at:at + n], cut=cut,
                     cull=args.cull)
        t1 = time.perf_counter()
        for at in range(0, len(cams), n):
            vol.integrate(cams[at:at + n], depths[at:at + n], normals[at:at + n],
                          images[at:at + n], cut=cut, grow=False)
        t2 = time.perf_counter()
        out = vol.extract()
        t3 = time.perf_counter()
    if times is not None:
        for k, v in (("mark", t1 - t0), ("integrate", t2 - t1), ("extract", t3 - t2)):
            times.setdefault(k, []).append(v)
    return out


def child(args):
    from smvs_amd import device
    c = case(args)
    for _ in range(CHILD_REPS):
        if args.batch and args.sparse:
            fuse_sparse_batched(c, args)
        elif args.batch:
            fuse_batched(c, args.batch, not args.no_cut)
        else:
            device.fuse_tsdf(*c, cut=not args.no_cut, **sparse_args(args))


def kernel_times(args):
    """-> {kernel: (launches per call, best total seconds per call)}"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "-o", "run",
               "--", sys.executable, os.path.abspath(__file__), "--child", "--dims",
               str(args.dims), "--views", str(args.views), "--size", str(args.size[0]),
               str(args.size[1])]
        if args.sparse:
            cmd += ["--sparse", "--max-bricks", str(args.max_bricks)]
        if args.cull:
            cmd += ["--cull"]
        if args.batch:
            cmd += ["--batch", str(args.batch)]
        if args.no_cut:
            cmd += ["--no-cut"]
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if res.returncode != 0:
            raise RuntimeError("rocprofv3 failed: " + res.stderr[-2000:])
        files = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            raise RuntimeError("rocprofv3 left no kernel trace")
        names = sparse_kernels(args) if args.sparse else KERNELS
        if args.batch:
            names = VOLUME_KERNELS
        if args.batch and args.sparse:
            names = SPARSE_VOLUME_KERNELS
            if args.cull:
                at = names.index("tsdf_sparse_seed_kernel")
                names = names[:at] + CULL_KERNELS + names[at + 1:]
        if args.no_cut or (args.batch == 1):
            names = [k for k in names if k != "mesh_cut_kernel"]
        rows = {k: [] for k in names}
        for fn in files:
            with open(fn) as f:
                for r in csv.DictReader(f):
                    for k in names:
                        if k in r["Kernel_Name"]:
                            rows[k].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    out = {}
    for k, v in rows.items():
        v.sort()
        if not v or len(v) % CHILD_REPS:
            raise RuntimeError("%d launches of %s in the trace of %d calls"
                               % (len(v), k, CHILD_REPS))
        per = len(v) // CHILD_REPS
        out[k] = (per, min(sum(1e-9 * (e - s) for s, e in v[i * per:(i + 1) * per])
                           for i in range(CHILD_REPS)))
    return out


def sparse_kernel_lines(args, kt, stats, n_vox):
    for k in sparse_kernels(args):
        per, t = kt[k]
        rec = {"case": "sparse_kernel", "kernel": k, "launches_per_call": per,
               "ms_per_call_best": round(1e3 * t, 4)}
        if k == "tsdf_sparse_seed_kernel":
            rec.update({"voxel_views": n_vox * args.views,
                        "ns_per_1000_voxel_views": round(1e12 * t / (n_vox * args.views), 4)})
        if k == "tsdf_sparse_seed_list_kernel" and stats["tested_bricks"]:
            pairs = 256 * stats["tested_bricks"] * args.views
            rec.update({"voxel_views": pairs,
                        "ns_per_1000_voxel_views": round(1e12 * t / pairs, 4)})
        if k == "tsdf_cull_kernel":
            pairs = stats["bricks"] * args.views
            rec.update({"brick_views": pairs,
                        "ns_per_1000_brick_views": round(1e12 * t / pairs, 3)})
        if k == "tsdf_sparse_integrate_kernel" and stats["allocated_bricks"]:
            pairs = 256 * stats["allocated_bricks"] * args.views
            rec.update({"voxel_views": pairs,
                        "ns_per_1000_voxel_views": round(1e12 * t / pairs, 3)})
        print(json.dumps(rec), flush=True)
    print(json.dumps({"case": "sparse_kernels_total",
                      "ms_per_call_best": round(1e3 * sum(t for _, t in kt.values()), 3)}),
          flush=True)


def batched_lines(args, c):
    """--batch: the one-shot entry and the batched volume, alternating"""
    import copy
    from smvs_amd import device
    cut = not args.no_cut
    n_vox = args.dims ** 3
    one, bat = [], []
    for _ in range(args.reps + 1):
        t0 = time.perf_counter()
        a = device.fuse_tsdf(*c, cut=cut)
        one.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        b = fuse_batched(c, args.batch, cut)
        bat.append(time.perf_counter() - t0)
    same = all(np.array_equal(a[k], b[k]) for k in a)
    if not cut and not same:
        raise SystemExit("tsdf_bench: without the cut the batched mesh must be the one-shot's")
    batches = -(-args.views // args.batch)
    print(json.dumps({"case": "batched_entry", "dims": [args.dims] * 3, "views": args.views,
                      "size": args.size, "cut": cut, "batch": args.batch, "batches": batches,
                      "same_mesh": bool(same), "vertices": len(b["xyz"]), "faces": len(b["faces"]),
                      "one_shot_ms_best": round(1e3 * min(one[1:]), 2),
                      "batched_ms_best": round(1e3 * min(bat[1:]), 2),
                      "state_bytes": 24 * n_vox}), flush=True)
    if args.no_kernels:
        return
    one_args = copy.copy(args)
    one_args.batch = 0
    for label, a in (("one_shot", one_args), ("batched", args)):
        kt = kernel_times(a)
        for k, (per, t) in kt.items():
            print(json.dumps({"case": label + "_kernel", "kernel": k, "launches_per_call": per,
                              "ms_per_call_best": round(1e3 * t, 4)}), flush=True)
        print(json.dumps({"case": label + "_kernels_total",
                          "ms_per_call_best": round(1e3 * sum(t for _, t in kt.values()), 3)}),
              flush=True)


def sparse_batched_lines(args, c):
    """--sparse --batch: the one-shot sparse entry and the persistent brick-sparse
    volume, alternating"""
    import copy
    from smvs_amd import device
    cut = not args.no_cut
    one, bat, phases = [], [], {}
    for _ in range(args.reps + 1):
        t0 = time.perf_counter()
        a = device.fuse_tsdf(*c, cut=cut, **sparse_args(args))
        one.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        b = fuse_sparse_batched(c, args, phases)
        bat.append(time.perf_counter() - t0)
    keys = ("xyz", "normals", "rgb", "confidence", "faces", "cells")
    same = all(np.array_equal(a[k], b[k]) for k in keys)
    if not cut and not same:
        raise SystemExit("tsdf_bench: without the cut the batched mesh must be the one-shot's")
    rec = {"case": "sparse_batched_entry", "dims": [args.dims] * 3, "views": args.views,
           "size": args.size, "cut": cut, "cull": bool(args.cull), "batch": args.batch,
           "batches": -(-args.views // args.batch), "same_mesh": bool(same),
           "vertices": len(b["xyz"]), "faces": len(b["faces"]),
           "one_shot_ms_best": round(1e3 * min(one[1:]), 2),
           "batched_ms_best": round(1e3 * min(bat[1:]), 2)}
    for k, v in phases.items():
        rec[k + "_ms_best"] = round(1e3 * min(v[1:]), 2)
    rec.update(b["stats"])
    print(json.dumps(rec), flush=True)
    if args.no_kernels:
        return
    one_args = copy.copy(args)
    one_args.batch = 0
    for label, a in (("one_shot", one_args), ("batched", args)):
        kt = kernel_times(a)
        for k, (per, t) in kt.items():
            print(json.dumps({"case": label + "_kernel", "kernel": k, "launches_per_call": per,
                              "ms_per_call_best": round(1e3 * t, 4)}), flush=True)
        print(json.dumps({"case": label + "_kernels_total",
                          "ms_per_call_best": round(1e3 * sum(t for _, t in kt.values()), 3)}),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--dims", type=int, default=256)
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--size", type=int, nargs=2, default=[960, 540])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--no-peaks", action="store_true")
    ap.add_argument("--sparse", action="store_true", help="smvs_tsdf_fuse_sparse")
    ap.add_argument("--resolution", type=int, help="with --sparse: --dims, up to 4096")
    ap.add_argument("--max-bricks", type=int, default=0)
    ap.add_argument("--cull", action="store_true",
                    help="with --sparse: the brick cull in front of the seed pass")
    ap.add_argument("--batch", type=int, default=0,
                    help="the persistent volume (with --sparse: the brick-sparse one), N views per "
                         "batch, against the one-shot")
    ap.add_argument("--no-cut", action="store_true", help="with --batch: the cut off")
    args = ap.parse_args()
    if args.batch < 0:
        ap.error("--batch must not be negative")
    if args.no_cut and not args.batch and not args.child:
        ap.error("--no-cut belongs to --batch")
    if args.cull and not args.sparse:
        ap.error("--cull belongs to --sparse")
    if args.resolution is not None:
        if not args.sparse:
            ap.error("--resolution belongs to --sparse")
        args.dims = args.resolution
    if args.child:
        child(args)
        return
    import smvs_amd
    from smvs_amd import device
    if smvs_amd.device_count() < 1:
        raise SystemExit("tsdf_bench needs a GPU")
    c = case(args)
    if args.batch and args.sparse:
        sparse_batched_lines(args, c)
        return
    if args.batch:
        batched_lines(args, c)
        return
    n_vox = args.dims ** 3
    times = []
    for _ in range(args.reps + 1):
        t0 = time.perf_counter()
        out = device.fuse_tsdf(*c, cut=True, **sparse_args(args))
        times.append(time.perf_counter() - t0)
    pixels = args.size[0] * args.size[1] * args.views
    entry = {"case": "sparse_entry" if args.sparse else "entry", "dims": [args.dims] * 3,
             "views": args.views, "size": args.size, "cut": True, "vertices": len(out["xyz"]),
             "faces": len(out["faces"]), "fuse_ms_first": round(1e3 * times[0], 2),
             "fuse_ms_best": round(1e3 * min(times[1:]), 2)}
    if args.sparse:
        st = out["stats"]
        entry.update(st)
        if args.cull:
            from smvs_amd.device import pyramid_bytes
            entry.update({"cull": True,
                          "tested_share": round(st["tested_bricks"] / st["bricks"], 5),
                          "pyramid_bytes": args.views * pyramid_bytes(*args.size)})
        entry.update({"max_bricks": args.max_bricks or 1 << 20,
                      "allocated_share": round(st["allocated_bricks"] / st["bricks"], 5),
                      "dense_state_bytes": 28 * n_vox})
    print(json.dumps(entry), flush=True)
    if args.no_kernels:
        return
    kt = kernel_times(args)
    if args.sparse:
        sparse_kernel_lines(args, kt, out["stats"], n_vox)
        return
    copy_peak = None
    if not args.no_peaks:
        import peaks
        copy_peak = peaks.run()["hbm_copy_GBps"]
    for k in KERNELS:
        per, t = kt[k]
        rec = {"case": "kernel", "kernel": k, "launches_per_call": per,
               "ms_per_call_best": round(1e3 * t, 4)}
        if k == "tsdf_integrate_kernel":
            moved = 24 * n_vox + 4 * pixels
            rec.update({"voxel_views": n_vox * args.views,
                        "ns_per_1000_voxel_views": round(1e12 * t / (n_vox * args.views), 3),
                        "bytes_moved_MB": round(1e-6 * moved, 1),
                        "GBps": round(1e-9 * moved / t, 1)})
            if copy_peak:
                rec["hbm_copy_peak_GBps"] = round(copy_peak, 1)
                rec["fraction_of_hbm_copy_peak"] = round(1e-9 * moved / t / copy_peak, 4)
        print(json.dumps(rec), flush=True)
    print(json.dumps({"case": "kernels_total",
                      "ms_per_call_best": round(1e3 * sum(t for _, t in kt.values()), 3)}),
          flush=True)


if __name__ == "__main__":
    main()
