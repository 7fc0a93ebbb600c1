#!/usr/bin/env python3
"""Synthetic accuracy of the SGM front ends, on the CPU from the oracle and the
restatements under tests/ (no device): the sphere and the plane scene of
synth.pipeline_inputs at 384 x 256 with six neighbours, SGM scale 1 (192 x 128),
64 planes over the main view's depth range.  For the two-neighbour reference,
the consensus merge at n = 4 and 6 (0.95, 2) and the plane sweep at n = 2, 4
and 6 (defaults for n), without and with the support test: the coverage (share
of pixels with a depth) and, among those, the share whose depth lies within one
plane of the true depth (both taken to the nearest plane in inverse depth; the
truth is the mean of the four full-resolution pixels).  Behind those rows, for
the sweep with the support test at n = 4 and 6: the same with the two filters of
include/smvs_hip.h (the uniqueness test at 10 %, window 1, in front of the
support test; the speckle removal at ratio 0.95, size 200, behind it), each alone
and both, with the number of pixels whose depth is more than one plane off.

    python tools/sgm_sweep_accuracy.py > profiles/sgm_filters_synth_accuracy.txt

(profiles/sgm_sweep_synth_accuracy.txt holds the rows above the filters', from
before there were filters.)

Two synthetic scenes say nothing about real data."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import sgm_filter_ref as filter_ref
import sgm_merge_ref as merge_ref
import sgm_sweep_compose as compose
import sgm_sweep_ref as sweep_ref
from oracle import pyoracle as oracle
from smvs_amd import host, synth

D = 64
N = 6
UNIQUENESS, WINDOW, SPECKLE_SIZE, SPECKLE_RATIO = 10, 1, 200, 0.95


def checked_maps(inputs, n):
    """the n left/right-checked forward maps of the main view (2 n runs)"""
    imgs = [host.sgm_image(inputs, k, 1) for k in range(n + 1)]
    small = dict(inputs, images=imgs)

    def run(a, b, M, t, rng):
        depths = oracle.sgm_depths(rng[0], rng[1], D)
        sgm = oracle.sgm_aggregate(oracle.sgm_cost_volume(a, b, M, t, depths), 6, 96)
        return oracle.sgm_depth_from_volume(sgm, a, depths)[0]
    maps = []
    for k in range(1, n + 1):
        Mf, tf = host.view_reprojection(small, 0, k)
        Mb, tb = host.view_reprojection(small, k, 0)
        fwd = run(imgs[0], imgs[k], Mf, tf, host.depth_range(inputs, 0))
        bwd = run(imgs[k], imgs[0], Mb, tb, host.depth_range(inputs, k))
        maps.append(oracle.sgm_lr_check(fwd, bwd, Mf, tf))
    return np.stack(maps)


def main():
    print("# synthetic scenes of synth.pipeline_inputs(kind, 384, 256, 6, flen=1.2), SGM scale 1")
    print("# (192 x 128), %d planes; CPU oracle + restatements (tools/sgm_sweep_accuracy.py)" % D)
    print("# coverage: pixels with a depth; within: of those, depth within one plane of the truth")
    print("# Synthetic: two rendered scenes say nothing about real data.")
    filtered = []     # the rows of the filters, printed behind the others
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

        def row(name, depth, keep=None):
            valid = depth != 0
            near = np.abs(plane(np.where(valid, depth, 1.0).astype(np.float64)) - true_plane) <= 1
            text = ("%-7s %-46s coverage %5.1f %%  within %5.1f %%"
                    % (kind, name, 100.0 * valid.mean(), 100.0 * near[valid].mean()))
            if keep is None:
                print(text)
            else:
                keep.append(text + "  wrong %5d" % int((valid & ~near).sum()))
        print("# %s: depth range %.3f .. %.3f" % (kind, rng[0], rng[1]))
        stack = checked_maps(inputs, N)
        row("reference merge, n = 2", merge_ref.reference_merge(stack[0], stack[1]))
        for n in (4, 6):
            row("consensus (0.95, 2), n = %d" % n, merge_ref.consensus(stack[:n], 0.95, 2)[0])
        vols = compose.neighbour_volumes(oracle, main_img, nbs, rng, D)
        one = compose.sweep(oracle, main_img, nbs[:1], rng, D, vols=vols[:1])
        row("one neighbour, unchecked", one["unchecked"])
        for n in (2, 4, 6):
            min_views, best_k, support_cost, min_support = min(2, n), (n + 1) // 2, 20, min(2, n)
            got = compose.sweep(oracle, main_img, nbs[:n], rng, D, False, False, min_views, best_k,
                                support_cost, min_support, vols=vols[:n])
            row("sweep n = %d (min_views %d, best_k %d)" % (n, min_views, best_k),
                got["unchecked"])
            row("sweep n = %d, support (cost <= %d, >= %d)" % (n, support_cost, min_support),
                got["depth"])
            if n == 2:
                continue
            rejected = filter_ref.uniqueness(got["sgm"], got["argmin"], UNIQUENESS, WINDOW)[0]
            unique = sweep_ref.apply_support(
                filter_ref.apply_uniqueness(got["unchecked"], rejected), got["support"],
                min_support)
            row("sweep n = %d, support" % n, got["depth"], filtered)
            row("sweep n = %d, support, uniqueness" % n, unique, filtered)
            row("sweep n = %d, support, speckle" % n,
                filter_ref.filter_speckles(got["depth"], SPECKLE_SIZE, SPECKLE_RATIO)[0],
                filtered)
            row("sweep n = %d, support, uniqueness, speckle" % n,
                filter_ref.filter_speckles(unique, SPECKLE_SIZE, SPECKLE_RATIO)[0], filtered)
    print("# the sweep with the filters: uniqueness %d %%, window %d; speckle ratio %g, size %d;"
          % (UNIQUENESS, WINDOW, SPECKLE_RATIO, SPECKLE_SIZE))
    print("# wrong: pixels with a depth more than one plane off.  Synthetic, as above: this says")
    print("# nothing about real data.")
    for text in filtered:
        print(text)


if __name__ == "__main__":
    main()
