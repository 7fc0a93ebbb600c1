#!/usr/bin/env python3
"""Wall-clock breakdown of the C++ host DepthOptimizer::optimize on a
synthetic scene (SMVS_HOST_TIMING prints the per-phase split on stderr).
    host_optimize_timing.py [sphere|plane] W H N [--sgm [--subplane]]
--sgm: the SGM front end (scale 1, 128 planes) initialises the view, as
smvsrecon does by default; --subplane: with the sub-plane winner
(SGMStereo::Options::subplane).  With --sgm the batch log is also summed per
scale: Newton steps, active patch-steps, PCG iterations."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["SMVS_HOST_TIMING"] = "1"
import numpy as np
from smvs_amd import synth, host

args = [a for a in sys.argv[1:] if not a.startswith("--")]
kind = args[0] if len(args) > 0 else "sphere"
w = int(args[1]) if len(args) > 1 else 1920
h = int(args[2]) if len(args) > 2 else 1080
n = int(args[3]) if len(args) > 3 else 8
use_sgm = "--sgm" in sys.argv
subplane = "--subplane" in sys.argv
t = time.perf_counter()
inp = synth.pipeline_inputs(kind, w, h, n, flen=1.2 if kind == "sphere" else 1.0)
print("inputs rendered in %.1f s" % (time.perf_counter() - t))
sgm = None
if use_sgm:
    for rep in range(2):
        t = time.perf_counter()
        sgm = host.sgm_depth(inp, sgm_scale=1, subplane=subplane)
        dt = time.perf_counter() - t
        print("sgm front end%s: %.3f s, valid %.1f%%, %d distinct depths"
              % (" (sub-plane)" if subplane else "", dt, 100.0 * (sgm > 0).mean(),
                 np.unique(sgm[sgm > 0]).size))
for rep in range(2):
    t = time.perf_counter()
    out = host.optimize(inp, min_scale=2, sgm_depth=sgm)
    dt = time.perf_counter() - t
    d = out["depth"]; m = d > 0
    err = np.sqrt(np.mean((d[m] - inp["truth"][m]) ** 2)) if m.any() else float("nan")
    print("optimize: %.3f s, %d batches, valid px %.1f%%, depth rms %.4g" % (dt, len(out["log"]), 100.0 * m.mean(), err))
print(out["log"])
if use_sgm:
    log = out["log"]
    for scale in sorted({e["scale"] for e in log}, reverse=True):
        rows = [e for e in log if e["scale"] == scale]
        print("scale %d: %d batches, %d Newton steps, %d active patch-steps, %d PCG iterations"
              % (scale, len(rows), sum(e["newton_steps"] for e in rows),
                 sum(e["active_patch_steps"] for e in rows),
                 sum(e["cg_iterations"] for e in rows)))
    print("total: %d Newton steps, %d active patch-steps, %d PCG iterations, %d valid pixels"
          % (sum(e["newton_steps"] for e in log), sum(e["active_patch_steps"] for e in log),
             sum(e["cg_iterations"] for e in log), int(m.sum())))
