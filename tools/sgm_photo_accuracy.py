#!/usr/bin/env python3
"""Synthetic accuracy of the multi-view photo-consistency test of
include/smvs_hip.h behind the three SGM front ends, on the CPU from the oracle
and the restatements under tests/ (no device): the scenes, the plane count, the
truth and the two measures of tools/sgm_sweep_accuracy.py (coverage; of the
pixels with a depth the share within one plane of the truth), plus the number of
pixels whose depth is more than one plane off.  The test runs on each front's
final map with all six neighbours as witnesses, window radius 2, once as the mean
of the best 2 with at least 2 views and once as the mean of the best 3 with at
least 3, score >= 0.49 (an NCC of 0.7); where a row says so the speckle removal
(ratio 0.95) follows it.

    python tools/sgm_photo_accuracy.py > profiles/sgm_photo_synth_accuracy.txt

Two synthetic scenes say nothing about real data, and the options are untuned."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import sgm_filter_ref as filter_ref
import sgm_merge_ref as merge_ref
import sgm_photo_ref as photo_ref
import sgm_sweep_compose as compose
import sgm_sweep_ref as sweep_ref
from oracle import pyoracle as oracle
from sgm_sweep_accuracy import (D, N, SPECKLE_RATIO, SPECKLE_SIZE, UNIQUENESS, WINDOW,
                                checked_maps)
from smvs_amd import synth

RADIUS, MIN_SCORE, PHOTO_SPECKLE = 2, 0.49, 50
VARIANTS = ((2, 2), (3, 3))     # (best_k, min_views)


def main():
    print("# synthetic scenes of synth.pipeline_inputs(kind, 384, 256, 6, flen=1.2), SGM scale 1")
    print("# (192 x 128), %d planes; CPU oracle + restatements (tools/sgm_photo_accuracy.py)" % D)
    print("# coverage: pixels with a depth; within: of those, depth within one plane of the truth;")
    print("# wrong: pixels with a depth more than one plane off")
    print("# photo (k, v): the photo-consistency test with all %d neighbours as witnesses, radius %d,"
          % (N, RADIUS))
    print("# mean of the best k, at least v views, score >= %g; speckle S: the speckle removal at"
          % MIN_SCORE)
    print("# ratio %g, size S, behind it.  Untuned options." % SPECKLE_RATIO)
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
            valid = depth != 0
            near = np.abs(plane(np.where(valid, depth, 1.0).astype(np.float64)) - true_plane) <= 1
            print("%-7s %-52s coverage %5.1f %%  within %5.1f %%  wrong %5d"
                  % (kind, name, 100.0 * valid.mean(), 100.0 * near[valid].mean(),
                     int((valid & ~near).sum())))

        def rows(name, depth, speckle):
            row(name, depth)
            score, defined = photo_ref.scores(main_img, depth, nbs, RADIUS)
            for best_k, min_views in VARIANTS:
                kept = photo_ref.fold(depth, score, defined, best_k, min_views, MIN_SCORE)[0]
                row("  + photo (%d, %d)" % (best_k, min_views), kept)
                if speckle:
                    row("  + photo (%d, %d) + speckle %d" % (best_k, min_views, PHOTO_SPECKLE),
                        filter_ref.filter_speckles(kept, PHOTO_SPECKLE, SPECKLE_RATIO)[0])
        print("# %s: depth range %.3f .. %.3f" % (kind, rng[0], rng[1]))
        stack = checked_maps(inputs, N)
        rows("reference merge, n = 2", merge_ref.reference_merge(stack[0], stack[1]), True)
        rows("consensus (0.95, 2), n = %d" % N, merge_ref.consensus(stack, 0.95, 2)[0], False)
        min_views, best_k, support_cost, min_support = min(2, N), (N + 1) // 2, 20, min(2, N)
        got = compose.sweep(oracle, main_img, nbs, rng, D, False, False, min_views, best_k,
                            support_cost, min_support)
        rows("sweep n = %d, support" % N, got["depth"], False)
        rejected = filter_ref.uniqueness(got["sgm"], got["argmin"], UNIQUENESS, WINDOW)[0]
        unique = sweep_ref.apply_support(
            filter_ref.apply_uniqueness(got["unchecked"], rejected), got["support"], min_support)
        row("sweep n = %d, support, uniqueness %d, speckle %d" % (N, UNIQUENESS, SPECKLE_SIZE),
            filter_ref.filter_speckles(unique, SPECKLE_SIZE, SPECKLE_RATIO)[0])


if __name__ == "__main__":
    main()
