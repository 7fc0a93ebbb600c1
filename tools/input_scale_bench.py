#!/usr/bin/env python3
"""Times the input scaling of app/smvsrecon.cc:621-650 at 6000x4000x3 with two
halvings, 4000x3000x3 with one and 1920x1080x3 with one: the host function
(rescale_half_size_gaussian of csrc/host/scene_io.cc, one core), the device
entry end to end (smvs_rescale_half_gaussian: staging copy, upload, kernels,
download), and the kernels alone -- from the kernel trace of a child process
that runs the device entry under rocprofv3 (--no-kernels skips it).  Prints
one JSON line per case; the kernel lines carry the achieved fraction of the
HBM copy peak tools/peaks.py measures on the same GPU (--no-peaks: left out),
with the algorithmic bytes of a level: its input plus its output.

    python tools/input_scale_bench.py [--no-kernels] [--no-peaks] [--reps N]
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

CASES = [(6000, 4000, 3, 2), (4000, 3000, 3, 1), (1920, 1080, 3, 1)]
KERNEL = "rescale_half_gaussian_u8_kernel"
CHILD_REPS = 5


def image(w, h, c):
    return np.random.default_rng(w + h).integers(0, 256, (h, w, c)).astype(np.uint8)


def levels(w, h, c, halvings):
    """(input bytes, output bytes) of every level of a chain"""
    out = []
    for _ in range(halvings):
        nw, nh = (w + 1) // 2, (h + 1) // 2
        out.append((w * h * c, nw * nh * c))
        w, h = nw, nh
    return out


def child():
    """the device entry alone, CHILD_REPS times per case in CASES' order"""
    from smvs_amd import device
    for w, h, c, halvings in CASES:
        a = image(w, h, c)
        for _ in range(CHILD_REPS):
            device.rescale_half_gaussian(a, halvings)


def kernel_times():
    """-> per case, per level: the best kernel time in seconds of the child's
    launches (its launches come in CASES' order, CHILD_REPS chains per case)"""
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
    want = sum(CHILD_REPS * halvings for _, _, _, halvings in CASES)
    if len(rows) != want:
        raise RuntimeError("%d launches of %s in the trace, %d expected" % (len(rows), KERNEL, want))
    out, at = [], 0
    for _, _, _, halvings in CASES:
        best = [None] * halvings
        for _ in range(CHILD_REPS):
            for lvl in range(halvings):
                t = 1e-9 * (rows[at][1] - rows[at][0])
                best[lvl] = t if best[lvl] is None else min(best[lvl], t)
                at += 1
        out.append(best)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--no-peaks", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    if args.child:
        child()
        return
    import smvs_amd
    from smvs_amd import device, host
    if smvs_amd.device_count() < 1:
        raise SystemExit("input_scale_bench needs a GPU")
    for w, h, c, halvings in CASES:
        a = image(w, h, c)
        t_host = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            want = host.rescale_half_size_gaussian(a, halvings)
            t_host.append(time.perf_counter() - t0)
        t_dev = []
        for _ in range(args.reps + 1):
            t0 = time.perf_counter()
            got = device.rescale_half_gaussian(a, halvings)
            t_dev.append(time.perf_counter() - t0)
        print(json.dumps({"case": "end_to_end", "size": [w, h, c], "halvings": halvings,
                          "host_one_core_ms_best": round(1e3 * min(t_host), 2),
                          "device_ms_first": round(1e3 * t_dev[0], 2),
                          "device_ms_best": round(1e3 * min(t_dev[1:]), 2),
                          "host_over_device": round(min(t_host) / min(t_dev[1:]), 2),
                          "equal": bool(np.array_equal(got, want))}), flush=True)
    if args.no_kernels:
        return
    times = kernel_times()
    copy_peak = None
    if not args.no_peaks:
        import peaks
        copy_peak = peaks.run()["hbm_copy_GBps"]
    for (w, h, c, halvings), best in zip(CASES, times):
        cw, ch = w, h
        for lvl, ((b_in, b_out), t) in enumerate(zip(levels(w, h, c, halvings), best)):
            rec = {"case": "kernel", "size": [cw, ch, c], "level": lvl + 1,
                   "kernel_us_best": round(1e6 * t, 1),
                   "algorithmic_MB": round(1e-6 * (b_in + b_out), 2),
                   "GBps": round(1e-9 * (b_in + b_out) / t, 1)}
            if copy_peak:
                rec["hbm_copy_peak_GBps"] = round(copy_peak, 1)
                rec["fraction_of_hbm_copy_peak"] = round(1e-9 * (b_in + b_out) / t / copy_peak, 3)
            print(json.dumps(rec), flush=True)
            cw, ch = (cw + 1) // 2, (ch + 1) // 2


if __name__ == "__main__":
    main()
