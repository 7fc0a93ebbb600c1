#!/usr/bin/env python3
"""What DepthOptimizer::Options::init_slants does to an optimisation, on two
synthetic scenes (needs a GPU).

    python tools/slant_init_effect.py > profiles/surface_planes_synth_effect.txt

synth.pipeline_inputs("plane" | "sphere", 640, 480, 4): the SGM front end with
photo_radius=2, refine_sweeps=3 (the other options at their defaults), then
optimize() with init_slants off and on.  Per batch: Newton steps, active
patch-steps, CG iterations.  For the initial and the final surface: median and
95th-percentile relative depth error and normal angle error against the scene's
truth (the truth's normals from central differences of its depth map, through
the formula of Surface::get_normal_map; pixels next to a pixel without truth
are left out).  The initial surface is Surface::create at the optimiser's
initial scale from the filtered map and the slant plane of a context fed with
the front end's outputs.

Two rendered scenes say nothing about real data, and the option is untuned."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import smvs_amd
from smvs_amd import host, synth

W, H, N = 640, 480, 4


def truth_normals(truth, flen):
    inv_flen = 1.0 / (flen * max(W, H))
    t = truth.astype(np.float64)
    wx = np.zeros_like(t)
    wy = np.zeros_like(t)
    wx[:, 1:-1] = 0.5 * (t[:, 2:] - t[:, :-2])
    wy[1:-1, :] = 0.5 * (t[2:, :] - t[:-2, :])
    ok = np.zeros(t.shape, bool)
    v = t > 0
    ok[1:-1, 1:-1] = (v[1:-1, 1:-1] & v[1:-1, 2:] & v[1:-1, :-2] & v[2:, 1:-1] & v[:-2, 1:-1])
    yy, xx = np.mgrid[0:H, 0:W]
    x = xx + 0.5 - W / 2.0
    y = yy + 0.5 - H / 2.0
    nz = (x * wx + y * wy + t) * inv_flen
    n = np.stack([wx, -wy, nz], axis=-1)
    n /= np.maximum(np.linalg.norm(n, axis=-1, keepdims=True), 1e-300)
    return n, ok


def errors(depth, normals, truth, tn, tok):
    m = (depth > 0) & tok
    rel = np.abs(depth[m].astype(np.float64) / truth[m] - 1.0)
    cos = np.clip((normals[m].astype(np.float64) * tn[m]).sum(axis=-1), -1.0, 1.0)
    ang = np.degrees(np.arccos(cos))
    return (100.0 * m.mean(), 100.0 * np.median(rel), 100.0 * np.percentile(rel, 95),
            np.median(ang), np.percentile(ang, 95))


def main():
    if smvs_amd.device_count() < 1:
        raise SystemExit("needs a GPU")
    print("# tools/slant_init_effect.py: synth.pipeline_inputs(kind, %d, %d, %d), SGM scale 1," % (W, H, N))
    print("# front end with photo_radius=2, refine_sweeps=3, other options at their defaults;")
    print("# optimize(regularization=0.01, num_iterations=5, min_scale=2, sgm_depth, sgm_slant)")
    print("# with init_slants off and on.  pixels: share of the image with a surface and a truth")
    print("# normal; depth: relative depth error in percent; normal: angle to the truth's normal in")
    print("# degrees; median / 95th percentile.  batch rows: scale, iteration, Newton steps,")
    print("# active patch-steps, CG iterations, valid patches.")
    print("# Synthetic: two rendered scenes say nothing about real data; the option is untuned")
    print("# and stays off by default.")
    for kind in ("plane", "sphere"):
        inputs = synth.pipeline_inputs(kind, W, H, N)
        flen = inputs["cams"][0].flen
        truth = np.asarray(inputs["truth"], dtype=np.float32)
        tn, tok = truth_normals(truth, flen)
        sgm, conf, slant = host.sgm_depth(inputs, sgm_scale=1, photo_radius=2, refine_sweeps=3)
        fin = np.isfinite(slant).all(axis=-1) & (sgm > 0)
        print("%s: SGM map %d x %d, %.1f %% with a depth; slants median |gx| %.3g |gy| %.3g"
              % (kind, sgm.shape[1], sgm.shape[0], 100.0 * (sgm > 0).mean(),
                 np.median(np.abs(slant[fin][:, 0])), np.median(np.abs(slant[fin][:, 1]))))
        init_scale = int(max(np.ceil(np.log2(W * H / 1.7e6) / 2) + 4, 4.0))
        ctx = smvs_amd.ViewContext(W, H, 1)
        ctx.upload_image(-1, inputs["images"][0])
        filtered = ctx.sgm_init_depth(sgm)
        plane = ctx.sgm_init_slants(slant)
        ctx.close()
        for on in (False, True):
            tag = "init_slants on " if on else "init_slants off"
            d0, n0 = host.surface_maps(inputs, init_scale, init_depth=filtered,
                                       init_slant=plane if on else None)
            out = host.optimize(inputs, regularization=0.01, num_iterations=5, min_scale=2,
                                sgm_depth=sgm, sgm_slant=slant, init_slants=on)
            for name, d, n in (("initial", d0, n0), ("final  ", out["depth"], out["normals"])):
                print("%s %s %s surface (scale %d): pixels %5.1f %%  depth %6.3f / %6.3f %%  "
                      "normal %6.2f / %6.2f deg"
                      % ((kind, tag, name, init_scale if name == "initial" else 2)
                         + errors(d, n, truth, tn, tok)))
            tot = [0, 0, 0]
            for e in out["log"]:
                print("%s %s   batch scale %d iter %d: newton %3d  active patch-steps %8d  cg %5d  "
                      "valid %6d" % (kind, tag, e["scale"], e["iter"], e["newton_steps"],
                                     int(e["active_patch_steps"]), e["cg_iterations"],
                                     e["valid_patches"]))
                tot[0] += e["newton_steps"]
                tot[1] += int(e["active_patch_steps"])
                tot[2] += e["cg_iterations"]
            print("%s %s   total: newton %d  active patch-steps %d  cg %d" % ((kind, tag) + tuple(tot)))


if __name__ == "__main__":
    main()
