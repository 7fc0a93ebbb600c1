#!/usr/bin/env python3
"""Times the preparation of the main view's shading planes (StereoView::
initialize_linear, lib/stereo_view.cc:64-84) at 1920x1080x3, without and with
--gamma-srgb: the host path -- host.shading_planes (a view from the bytes, the
byte -> float conversion, the curve, the luminance, the quadratic fit on one
core, the planes copied out) and the smvs_ctx_upload_shading call that follows
it in DepthOptimizer::upload_images -- against the device path:
smvs_ctx_prepare_shading from enqueue to smvs_ctx_synchronize, and its kernel
alone from the context's event timers (smvs_profile_*).  Prints one JSON line
per case; the planes of both paths are compared on the way.

    python tools/shading_prep_bench.py [--reps N] [--size W H C]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def best(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = fn()
        out.append(time.perf_counter() - t0)
    return min(out), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", type=int, nargs=3, default=[1920, 1080, 3])
    args = ap.parse_args()
    import smvs_amd
    from smvs_amd import device, host
    if smvs_amd.device_count() < 1:
        raise SystemExit("shading_prep_bench needs a GPU")
    w, h, c = args.size
    img = np.random.default_rng(w + h).integers(0, 256, (h, w, c)).astype(np.uint8)
    lut = host.gamma_inv_srgb_lut()
    ctx = device.ViewContext(w, h, 1)
    try:
        ctx.upload_image(-1, img)
        for gamma in (False, True):
            t_host, (want_s, want_g) = best(lambda: host.shading_planes(img, gamma=gamma),
                                            args.reps)

            def upload():
                ctx.upload_shading(want_s, want_g)      # (synchronises itself)
            ctx.synchronize()
            t_upload, _ = best(upload, args.reps)

            def prepare():
                ctx.prepare_shading(lut if gamma else None)
                ctx.synchronize()
            prepare()                                   # (first launch: code object load)
            t_dev, _ = best(prepare, args.reps)
            ctx.profile(True)
            kernel_ms = []
            for _ in range(args.reps):
                ctx.profile_reset()
                prepare()
                ms, launches = ctx.profile_get()["misc"]
                assert launches == 1
                kernel_ms.append(ms)
            ctx.profile(False)
            got_s, got_g = ctx.download_shading()
            algorithmic = w * h * (4 * c + 4 + 8)
            print(json.dumps({
                "size": [w, h, c], "gamma": gamma,
                "host_planes_one_core_ms_best": round(1e3 * t_host, 2),
                "upload_shading_ms_best": round(1e3 * t_upload, 2),
                "host_path_ms": round(1e3 * (t_host + t_upload), 2),
                "prepare_shading_to_synchronize_ms_best": round(1e3 * t_dev, 3),
                "kernel_us_best": round(1e3 * min(kernel_ms), 1),
                "kernel_algorithmic_MB": round(1e-6 * algorithmic, 1),
                "kernel_GBps": round(1e-9 * algorithmic / (1e-3 * min(kernel_ms)), 1),
                "host_path_over_device": round((t_host + t_upload) / t_dev, 1),
                "equal": bool(np.array_equal(got_s, want_s) and np.array_equal(got_g, want_g)),
            }), flush=True)
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
