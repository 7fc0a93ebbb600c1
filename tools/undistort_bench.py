#!/usr/bin/env python3
"""Times the undistortion resampling (smvs_undistort_u8) at 1920x1080x3 and
6000x4000x3 with an OPENCV lens: the host form (undistort_u8 of
csrc/host/colmap_io.cc, one core), the device entry end to end (staging copy,
upload, kernel, download), and the kernel alone -- from the kernel trace of a
child process that runs the device entry under rocprofv3 (--no-kernels skips
it).  Prints one JSON line per case; the kernel lines carry the bytes moved
(input + output) over the kernel time and the fraction of the HBM copy peak
tools/peaks.py measures on the same GPU (--no-peaks: left out).  --import times
one import of a four-view 1920x1080 ring (PNG in, PNG out) on the host form and
on the device and prints the stages' split.

    python tools/undistort_bench.py [--no-kernels] [--no-peaks] [--import] [--reps N]
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

CASES = [(1920, 1080, 3), (6000, 4000, 3)]
KERNEL = "undistort_u8_kernel"
CHILD_REPS = 5


def image(w, h, c):
    return np.random.default_rng(w + h).integers(0, 256, (h, w, c)).astype(np.uint8)


def lens(w, h):
    """An OPENCV lens in proportion to the image, mild barrel distortion."""
    m = float(max(w, h))
    return dict(fx=0.83 * m, fy=0.81 * m, cx=0.5 * w + 3.3, cy=0.5 * h - 2.2, k1=-0.12, k2=0.03,
                p1=0.001, p2=-0.002)


def child():
    """the device entry alone, CHILD_REPS times per case in CASES' order"""
    from smvs_amd import device
    for w, h, c in CASES:
        a = image(w, h, c)
        for _ in range(CHILD_REPS):
            device.undistort(a, lens(w, h), lens(w, h)["fx"])


def kernel_times():
    """-> per case the best kernel time in seconds of the child's launches"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "-o", "run",
               "--", sys.executable, os.path.abspath(__file__), "--child"]
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if res.returncode != 0:
            raise RuntimeError("rocprofv3 failed: " + res.stderr[-2000:])
        files = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            raise RuntimeError("rocprofv3 left no kernel trace")
        rows = []
        for fn in files:
            with open(fn) as f:
                for r in csv.DictReader(f):
                    if KERNEL in r["Kernel_Name"]:
                        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    rows.sort()
    if len(rows) != CHILD_REPS * len(CASES):
        raise RuntimeError("%d launches of %s in the trace, %d expected"
                           % (len(rows), KERNEL, CHILD_REPS * len(CASES)))
    return [min(1e-9 * (e - s) for s, e in rows[i * CHILD_REPS:(i + 1) * CHILD_REPS])
            for i in range(len(CASES))]


def import_split():
    """One import of a four-view 1920 x 1080 ring, host form and device"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import colmap_helpers as ch
    from smvs_amd import host, synth
    w, h = 1920, 1080
    main, subs = synth.ring_cameras(w, h, 3, flen=1.2)
    cams = [main] + subs
    m = float(w)
    params = [1.2 * m, 1.19 * m, 0.5 * w + 3.3, 0.5 * h - 2.2, -0.12, 0.03, 0.001, -0.002]
    model = ch.ring_model(cams, np.zeros((1, 3), np.float32), "OPENCV", params)
    with tempfile.TemporaryDirectory() as tmp:
        ch.write_binary(os.path.join(tmp, "model"), model)
        os.makedirs(os.path.join(tmp, "images"))
        for k, iid in enumerate(ch.ring_image_ids(4)):
            host.save_png(os.path.join(tmp, "images", model["images"][iid]["name"]),
                          image(w + k, h, 3)[:, :w])
        for name, dev in (("host", None), ("device", 0), ("device", 0)):
            rep = host.import_colmap(os.path.join(tmp, "model"), os.path.join(tmp, "images"),
                                     os.path.join(tmp, "scene"), device=dev, threads=4,
                                     overwrite=True)
            print(json.dumps({"case": "import_4x1920x1080x3_png", "undistort": name,
                              "threads": 4, "wall_s": round(rep["seconds"], 3),
                              "decode_s": round(rep["decode_seconds"], 3),
                              "undistort_s": round(rep["undistort_seconds"], 3),
                              "encode_s": round(rep["encode_seconds"], 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--no-peaks", action="store_true")
    ap.add_argument("--import", dest="do_import", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    if args.child:
        child()
        return
    import smvs_amd
    from smvs_amd import device, host
    if smvs_amd.device_count() < 1:
        raise SystemExit("undistort_bench needs a GPU")
    for w, h, c in CASES:
        a = image(w, h, c)
        L, focal = lens(w, h), lens(w, h)["fx"]
        t_host = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            want, want_blank = host.undistort(a, L, focal, return_blank=True)
            t_host.append(time.perf_counter() - t0)
        t_dev = []
        for _ in range(args.reps + 1):
            t0 = time.perf_counter()
            got, blank = device.undistort(a, L, focal, return_blank=True)
            t_dev.append(time.perf_counter() - t0)
        print(json.dumps({"case": "end_to_end", "size": [w, h, c],
                          "host_one_core_ms_best": round(1e3 * min(t_host), 2),
                          "device_ms_first": round(1e3 * t_dev[0], 2),
                          "device_ms_best": round(1e3 * min(t_dev[1:]), 2),
                          "host_over_device": round(min(t_host) / min(t_dev[1:]), 2),
                          "blank_pixels": blank,
                          "equal": bool(np.array_equal(got, want) and blank == want_blank)}),
              flush=True)
    if args.do_import:
        import_split()
    if args.no_kernels:
        return
    times = kernel_times()
    copy_peak = None
    if not args.no_peaks:
        import peaks
        copy_peak = peaks.run()["hbm_copy_GBps"]
    for (w, h, c), t in zip(CASES, times):
        moved = 2 * w * h * c
        rec = {"case": "kernel", "size": [w, h, c], "kernel_us_best": round(1e6 * t, 1),
               "bytes_moved_MB": round(1e-6 * moved, 2), "GBps": round(1e-9 * moved / t, 1)}
        if copy_peak:
            rec["hbm_copy_peak_GBps"] = round(copy_peak, 1)
            rec["fraction_of_hbm_copy_peak"] = round(1e-9 * moved / t / copy_peak, 3)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
