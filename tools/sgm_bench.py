#!/usr/bin/env python3
"""Times smvs_sgm_run on the 960x540x128 workload of BASELINE.json configs[2]
(profiling helper; use under rocprofv3 for per-kernel numbers).
--adaptive-p2: the adaptive-penalty aggregation (SMVS_SGM_P2_ADAPTIVE, the
reference's build without SSE) instead of the constant one; --subplane: the
sub-plane winner (SMVS_SGM_WINNER_SUBPLANE) instead of the plane's depth, and
the distinct depth values of the map; --repeat N: N timed
calls instead of 3; --num-steps N: N inverse-depth planes instead of 128
(2 .. 128, or a multiple of 8 from 136 to 256); --p2 N: penalty2 instead of 96
(above 255: the u16 volume with atomics); --kernels: after one warm-up call,
the per-kernel event times of the timed calls (smvs_sgm_profile) and the path
kernel's share of the HBM peak from its algorithmic bytes."""
import ctypes as C
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import smvs_amd
from smvs_amd import synth, _capi


def _arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


w, h = (1920, 1080) if "--small" not in sys.argv else (480, 270)
main, subs = synth.ring_cameras(w, h, 1)
scene = synth.SphereScene(px_size=3.0 / (1.2 * w))
imgs = [synth.render(scene, c) for c in (main, subs[0])]
half = [im[::2, ::2].copy() for im in imgs]  # stand-in for rescale_half_size
hw, hh = half[0].shape[1], half[0].shape[0]
cm = synth.Camera(main.R, main.t, main.flen, hw, hh)
cs = synth.Camera(subs[0].R, subs[0].t, subs[0].flen, hw, hh)
M, t = synth.reprojection(cm, cs)
adaptive = "--adaptive-p2" in sys.argv
repeat = _arg("--repeat", 3)
D = _arg("--num-steps", 128)
p2 = _arg("--p2", 96)
kernels = "--kernels" in sys.argv
subplane = "--subplane" in sys.argv
kw = dict(adaptive_p2=True) if adaptive else {}
if adaptive:
    print("penalty2 adapted to the intensity step (SMVS_SGM_P2_ADAPTIVE)")
if subplane:
    kw["subplane"] = True
    print("sub-plane winner (SMVS_SGM_WINNER_SUBPLANE)")


def run():
    return smvs_amd.sgm_run(half[0], half[1], M.astype(np.float32), t.astype(np.float32),
                            2.0, 10.0, D, 6, p2, **kw)


lib = _capi.load()
if kernels:
    run()   # warm-up: workspace growth, first-launch costs
    lib.smvs_sgm_profile(1, None, None)
for i in range(repeat):
    t0 = time.perf_counter()
    out = run()
    dt = time.perf_counter() - t0
    print("sgm_run %dx%dx%d: %.1f ms (incl. H2D/D2H), valid %.2f" % (hw, hh, D, 1e3 * dt, (out["depth"] > 0).mean()))
if subplane:
    print("distinct depth values: %d" % np.unique(out["depth"][out["depth"] > 0]).size)
if kernels:
    ms = (C.c_double * 8)()
    cnt = (C.c_longlong * 8)()
    lib.smvs_sgm_profile(0, ms, cnt)
    names = ["census", "warp", "cost", "paths", "wta"]
    for i, name in enumerate(names):
        if cnt[i]:
            print("kernel %-6s %9.1f us per call (%d launches)" % (name, 1e3 * ms[i] / cnt[i], cnt[i]))
    if cnt[3]:
        # each of the eight directions reads C once and writes one byte per cell
        # (penalty2 <= 255), or adds a u16 to S (read + write) otherwise
        cells = hw * hh * D
        nbytes = 8 * cells * (2 if p2 <= 255 else 5)
        us = 1e3 * ms[3] / cnt[3]
        print("paths: %.1f MB algorithmic, %.2f TB/s, %.2f of the 8 TB/s HBM peak"
              % (nbytes / 1e6, nbytes / us / 1e6, nbytes / us / 1e6 / 8.0))
