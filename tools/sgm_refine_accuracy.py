#!/usr/bin/env python3
"""Synthetic accuracy of the multi-view plane refinement sweeps of
include/smvs_hip.h behind the three SGM front ends, on the CPU from the oracle
and the restatements under tests/ (no device): the scenes, the plane count, the
truth and the measures of tools/sgm_photo_accuracy.py (coverage; of the pixels
with a depth the share within one plane of the truth; the pixels more than one
plane off), plus the median relative depth error of the pixels with a depth --
the staircase of the planes shows there, not in "within one plane".  Each front's
final map before and after: the photo test alone (radius 2, best 2 of at least 2,
score >= 0.49, all six neighbours as witnesses), then the sweeps in its place at
1, 2 and 3 sweeps with 2 samples and at 3 sweeps without samples, fill 1, the
other options at their defaults; one row with fill 0.

    python tools/sgm_refine_accuracy.py > profiles/sgm_refine_synth_accuracy.txt

Two synthetic scenes say nothing about real data, and the options are untuned."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import sgm_merge_ref as merge_ref
import sgm_refine_ref as refine_ref
import sgm_sweep_compose as compose
from oracle import pyoracle as oracle
from sgm_sweep_accuracy import D, N, checked_maps
from smvs_amd import synth

RADIUS, BEST_K, MIN_VIEWS, MIN_SCORE = 2, 2, 2, 0.49
VARIANTS = ((0, 2, 1), (1, 2, 1), (2, 2, 1), (3, 2, 1), (3, 0, 1), (3, 2, 0))  # sweeps, samples, fill


def main():
    print("# synthetic scenes of synth.pipeline_inputs(kind, 384, 256, 6, flen=1.2), SGM scale 1")
    print("# (192 x 128), %d planes; CPU oracle + restatements (tools/sgm_refine_accuracy.py)" % D)
    print("# coverage: pixels with a depth; within: of those, depth within one plane of the truth;")
    print("# wrong: pixels with a depth more than one plane off; median: the median relative depth")
    print("# error of the pixels with a depth")
    print("# photo: the photo-consistency test with all %d neighbours as witnesses, radius %d, mean of"
          % (N, RADIUS))
    print("# the best %d, at least %d views, score >= %g; refine (s, m, f): the plane refinement"
          % (BEST_K, MIN_VIEWS, MIN_SCORE))
    print("# sweeps in its place, s sweeps, m samples, fill f, depth_step 0.02, slant_step 0.01,")
    print("# seed 1.  Untuned options.")
    print("# Synthetic: two rendered scenes say nothing about real data.")
    for kind in ("sphere", "plane"):
        inputs = synth.pipeline_inputs(kind, 384, 256, N, flen=1.2)
        truth = inputs["truth"].astype(np.float64)
        truth = 0.25 * (truth[0::2, 0::2] + truth[1::2, 0::2] + truth[0::2, 1::2]
                        + truth[1::2, 1::2])
        main_img, nbs, rng = compose.front_end_inputs(inputs, N)
        inv = 1.0 / oracle.sgm_depths(rng[0], rng[1], D).astype(np.float64)

        def plane(depth):
            return np.abs(inv[None, None, :] - 1.0 / depth[:, :, None]).argmin(axis=2)
        true_plane = plane(truth)

        def row(name, depth):
            valid = depth > 0
            near = np.abs(plane(np.where(valid, depth, 1.0).astype(np.float64)) - true_plane) <= 1
            err = np.abs(depth[valid].astype(np.float64) / truth[valid] - 1.0)
            print("%-7s %-40s coverage %5.1f %%  within %5.1f %%  wrong %5d  median %6.3f %%"
                  % (kind, name, 100.0 * valid.mean(), 100.0 * near[valid].mean(),
                     int((valid & ~near).sum()), 100.0 * np.median(err)))

        def rows(name, depth):
            row(name, depth)
            for sweeps, samples, fill in VARIANTS:
                counts = {}
                out = refine_ref.plane_refine(main_img, depth, nbs, RADIUS, BEST_K, MIN_VIEWS,
                                              MIN_SCORE, sweeps=sweeps, samples=samples, fill=fill,
                                              counts=counts)[0]
                row("  + photo" if sweeps == 0 else
                    "  + refine (%d, %d, %d)" % (sweeps, samples, fill), out)
        print("# %s: depth range %.3f .. %.3f" % (kind, rng[0], rng[1]))
        stack = checked_maps(inputs, N)
        rows("reference merge, n = 2", merge_ref.reference_merge(stack[0], stack[1]))
        rows("consensus (0.95, 2), n = %d" % N, merge_ref.consensus(stack, 0.95, 2)[0])
        min_views, best_k, support_cost, min_support = min(2, N), (N + 1) // 2, 20, min(2, N)
        got = compose.sweep(oracle, main_img, nbs, rng, D, False, False, min_views, best_k,
                            support_cost, min_support)
        rows("sweep n = %d, support" % N, got["depth"])


if __name__ == "__main__":
    main()
