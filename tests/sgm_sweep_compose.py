"""The multi-neighbour plane sweep of the SGM front end composed from the
oracle's pieces and the restatements (tests/test_sgm_sweep_cpu.py,
tests/test_gpu_sgm_sweep.py): per neighbour oracle.sgm_cost_volume -> fold ->
oracle.sgm_aggregate (or the adaptive restatement) -> oracle.sgm_depth_from_volume
(or the sub-plane restatement) -> support."""
import numpy as np

import sgm_adaptive_ref as adaptive_ref  # tests/sgm_adaptive_ref.py
import sgm_subplane_ref as subplane_ref  # tests/sgm_subplane_ref.py
import sgm_sweep_ref as ref              # tests/sgm_sweep_ref.py


def front_end_inputs(inputs, n, halvings=1):
    """The SGM-scale images of the main view and its first n neighbours, the
    neighbours' reprojections main -> neighbour and the main view's depth range."""
    from smvs_amd import host
    imgs = [host.sgm_image(inputs, k, halvings) for k in range(n + 1)]
    small = dict(inputs, images=imgs)
    nbs = []
    for k in range(1, n + 1):
        M, t = host.view_reprojection(small, 0, k)
        nbs.append(dict(image=imgs[k], M_fwd=M, t_fwd=t))
    return imgs[0], nbs, host.depth_range(inputs, 0)


def neighbour_volumes(oracle, main, nbs, rng, D):
    """(n, h, w, D) u8: the cost volume of every pair over the main view's planes"""
    depths = oracle.sgm_depths(rng[0], rng[1], D)
    vols = np.stack([oracle.sgm_cost_volume(main, nb["image"], nb["M_fwd"], nb["t_fwd"], depths)
                     for nb in nbs])
    assert vols.max() <= 255
    return vols.astype(np.uint8)


def sweep(oracle, main, nbs, rng, D, adaptive=False, subplane=False, min_views=1, best_k=0,
          support_cost=20, min_support=0, p1=6, p2=96, vols=None):
    """dict(vols, cost, sgm, argmin, unchecked, support, depth): the composition."""
    if vols is None:
        vols = neighbour_volumes(oracle, main, nbs, rng, D)
    depths = oracle.sgm_depths(rng[0], rng[1], D)
    cost = ref.fold(vols, min_views, best_k)
    sgm = (adaptive_ref.aggregate(cost.astype(np.uint16), main, p1, p2, literal=False) if adaptive
           else oracle.sgm_aggregate(cost, p1, p2))
    plane, argmin = oracle.sgm_depth_from_volume(sgm, main, depths)
    unchecked = (subplane_ref.subplane_depth(sgm, argmin, main, rng[0], rng[1]) if subplane
                 else plane)
    sup = ref.support(vols, argmin, support_cost)
    return dict(vols=vols, cost=cost, sgm=sgm, argmin=argmin, unchecked=unchecked, support=sup,
                depth=ref.apply_support(unchecked, sup, min_support))
