"""GPU parity of the n-neighbour consensus merge of the SGM front end (DESIGN.md
section 3.6, "n-neighbour consensus"; SMVS_SGM_MERGE_CONSENSUS of
include/smvs_hip.h): the fused check-and-merge kernel on made-up maps against
oracle.sgm_lr_check and the numpy restatement tests/sgm_merge_ref.py, a view's
front end over four neighbours against the composition of the oracle's pieces,
the host mirror, the optimizer started from the merged map, and the scene run.
The definition fixes every float operation: every comparison of a map is
array_equal."""
import ctypes as C
import os

import numpy as np
import pytest

import sgm_adaptive_ref as adaptive_ref  # tests/sgm_adaptive_ref.py
import sgm_merge_ref as ref              # tests/sgm_merge_ref.py
import sgm_subplane_ref as subplane_ref  # tests/sgm_subplane_ref.py
from parity_units import assert_same_units  # tests/parity_units.py

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def hip():
    import smvs_amd
    if smvs_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on a GPU")
    return smvs_amd


# ---------------------------------------------------- the kernel on made-up maps
W, H = 70, 37
SIZES = [(70, 37), (64, 40), (33, 29)]          # (width, height) of the neighbours, cycled
LEVELS = np.array([2.0, 2.6, 3.4, 4.5], F)      # neighbouring levels: ratio 0.76 .. 0.77
JITTER = np.array([0.94, 0.97, 1.0, 1.03, 1.06], F)
SEED = 20


def made_up_maps(n, seed=SEED):
    """n forward maps of the W x H main view and, per neighbour, a backward map
    of its own size with a mild similarity main -> neighbour.  Depths: a level
    field shared by all maps (6 x 6 blocks of LEVELS) times a JITTER of +-6 %,
    one map in eight on another level; a quarter of every map is zero (4 x 4
    blocks, outside a window in the middle where all maps stay valid and on the
    shared level, so that full support occurs).  That gives clusters,
    near-threshold pairs and exact ties."""
    rng = np.random.default_rng(seed)
    blocks = rng.integers(0, LEVELS.size, ((H + 5) // 6, (W + 5) // 6))
    level = np.kron(blocks, np.ones((6, 6), np.int64))[:H, :W]
    safe = np.zeros((H, W), bool)
    safe[13:24, 26:44] = True

    def zero_mask(h, w, keep):
        z = rng.random(((h + 3) // 4, (w + 3) // 4)) < 0.29
        return np.kron(z, np.ones((4, 4), bool))[:h, :w] & ~keep

    fwd = np.zeros((n, H, W), F)
    nbs = []
    for k in range(n):
        nw, nh = SIZES[k % len(SIZES)]
        other = rng.random((H, W)) < 0.125
        lev = np.where(other & ~safe, (level + rng.integers(1, LEVELS.size, (H, W))) % LEVELS.size,
                       level)
        fwd[k] = LEVELS[lev] * JITTER[rng.integers(0, JITTER.size, (H, W))]
        fwd[k][zero_mask(H, W, safe)] = 0
        # main -> neighbour: scale to the neighbour's size and a little more, a
        # small rotation, an offset; t shifts by up to a pixel with the depth
        s = min(nw / W, nh / H) * (1.02 + 0.03 * (k % 4))
        ang = 0.03 * ((k % 5) - 2)
        ox = 0.5 * (nw - s * W) + 1.5 * ((k % 3) - 1)
        oy = 0.5 * (nh - s * H) + 1.0 * ((k % 2) * 2 - 1)
        M = np.array([[s * np.cos(ang), -s * np.sin(ang), ox],
                      [s * np.sin(ang), s * np.cos(ang), oy], [0, 0, 1]], F)
        t = np.array([1.5 * ((k % 2) * 2 - 1), -1.0, 0.05], F)
        # the backward map: the main view's level at the pixel that lands here
        py, px = np.mgrid[0:nh, 0:nw].astype(np.float64)
        inv = np.linalg.inv(M.astype(np.float64))
        mx = np.clip(np.rint(inv[0, 0] * px + inv[0, 1] * py + inv[0, 2]), 0, W - 1).astype(int)
        my = np.clip(np.rint(inv[1, 0] * px + inv[1, 1] * py + inv[1, 2]), 0, H - 1).astype(int)
        bwd = (LEVELS[level[my, mx]] * JITTER[rng.integers(0, JITTER.size, (nh, nw))]).astype(F)
        bwd[zero_mask(nh, nw, safe[my, mx])] = 0
        nbs.append(dict(bwd=bwd, M_fwd=M.reshape(9), t_fwd=t))
    return fwd, nbs


RATIOS = (0.0, 0.8, 0.95, 1.0)


def branch_counts(stack, ratio, min_agree):
    """How often the consensus goes each way on a stack of checked maps."""
    merged, support, best = ref.consensus(stack, ratio, min_agree)
    star = ref.stars(stack, ratio)
    n = stack.shape[0]
    valid = stack != 0
    count = star.sum(axis=1)                                # [k]: size of k's star
    mine = np.take_along_axis(star, best[None, None], axis=0)[0]   # [j]: j in the winning star
    first = np.argmax(valid, axis=0)
    any_valid = valid.any(axis=0)
    tie = np.zeros(best.shape, bool)
    for k in range(n):
        tie |= (count[k] == support) & (k != best) & any_valid & np.any(star[k] != mine, axis=0)
    return dict(winner_not_first=int((any_valid & (best != first)).sum()),
                valid_outside_star=int((valid & ~mine).any(axis=0).sum()),
                tie_by_order=int(tie.sum()),
                min_agree_rejects=int(((support > 0) & (support < min_agree)).sum()),
                full_support=int((support == n).sum()),
                merged_valid=int((merged != 0).sum()))


@pytest.mark.parametrize("n", [1, 2, 3, 5, 16])
def test_check_merge_kernel_on_made_up_maps(hip, oracle, n):
    """5. smvs_sgm_check_merge, neighbours of three different sizes, agree_ratio
    in {0, 0.8, 0.95, 1} x min_agree in {1, 2, n}: checked[k] is
    oracle.sgm_lr_check of map k, merged and support are the restatement's.
    Before comparing, the restatement alone shows that every branch occurs: a
    check rejected by the border, by the ratio and by a zero neighbour depth,
    a rejection by min_agree, full support n; for n >= 2 (one map has no choice
    to make) a valid map outside the winning star and a tie decided by order;
    for n >= 3 a winner that is not the first valid map (the stars of two maps
    have the same size, so the first valid one always wins)."""
    fwd, nbs = made_up_maps(n)
    assert abs((fwd == 0).mean() - 0.25) < 0.06
    want_checked = np.stack([oracle.sgm_lr_check(fwd[k], nbs[k]["bwd"], nbs[k]["M_fwd"],
                                                 nbs[k]["t_fwd"]) for k in range(n)])
    check = dict(border=0, zero_neighbor=0, ratio=0, kept=0)
    for k in range(n):
        b = ref.lr_check_branches(fwd[k], nbs[k]["bwd"], nbs[k]["M_fwd"], nbs[k]["t_fwd"])
        assert np.array_equal(b["kept"], want_checked[k] != 0)
        assert np.array_equal(want_checked[k][b["kept"]], fwd[k][b["kept"]])
        for key in check:
            check[key] += int(b[key].sum())
    print("n %d: checks %s" % (n, check))
    for key, value in check.items():
        assert value >= 1, key
    total = {}
    wants = {}
    for ratio in RATIOS:
        for min_agree in sorted({1, 2, n}):
            wants[(ratio, min_agree)] = ref.consensus(want_checked, ratio, min_agree)
            c = branch_counts(want_checked, ratio, min_agree)
            print("n %d ratio %.2f min_agree %d: %s" % (n, ratio, min_agree, c))
            for key, value in c.items():
                total[key] = total.get(key, 0) + value
    needed = ["min_agree_rejects", "full_support", "merged_valid"]
    if n >= 2:
        needed += ["valid_outside_star", "tie_by_order"]
    if n >= 3:
        needed += ["winner_not_first"]
    for key in needed:
        assert total[key] >= 1, key

    for (ratio, min_agree), (merged, support, _) in wants.items():
        got = hip.sgm_check_merge(fwd, nbs, agree_ratio=ratio, min_agree=min_agree)
        assert np.array_equal(got["checked"], want_checked), (ratio, min_agree)
        assert np.array_equal(got["merged"], merged), (ratio, min_agree)
        assert np.array_equal(got["support"], support), (ratio, min_agree)


# ------------------------------------------------------------ a view's front end
N_NEIGHBORS = 4
PLANES = 64


@pytest.fixture(scope="module")
def scene_inputs():
    from smvs_amd import synth
    return synth.pipeline_inputs("sphere", 384, 256, N_NEIGHBORS, flen=1.2)


def _front_end_inputs(inputs, n=N_NEIGHBORS):
    """The SGM-scale images, reprojections and depth ranges of the main view and
    its first n neighbours, as smvs_sgm_depth_for_view wants them
    (tests/test_gpu_sgm_subplane.py)."""
    from smvs_amd import host
    imgs = [host.sgm_image(inputs, k, 1) for k in range(n + 1)]
    small = dict(inputs, images=imgs)
    nbs = []
    for k in range(1, n + 1):
        Mf, tf = host.view_reprojection(small, 0, k)
        Mb, tb = host.view_reprojection(small, k, 0)
        nbs.append(dict(image=imgs[k], M_fwd=Mf, t_fwd=tf, M_bwd=Mb, t_bwd=tb,
                        range_main=host.depth_range(inputs, 0),
                        range_neighbor=host.depth_range(inputs, k)))
    return imgs[0], nbs


_CHECKED = {}


def _checked_maps(oracle, inputs, adaptive, subplane, D=PLANES, n=N_NEIGHBORS):
    """The n checked forward maps of the view: 2 n runs (oracle cost volume,
    oracle or adaptive-restatement aggregation, oracle winners, refined by the
    sub-plane restatement when asked for) and oracle.sgm_lr_check; computed once
    per mode."""
    key = (tuple(inputs["view_ids"]), adaptive, subplane, D, n)
    if key not in _CHECKED:
        main, nbs = _front_end_inputs(inputs, n)

        def run(a, b, M, t, rng):
            depths = oracle.sgm_depths(rng[0], rng[1], D)
            cost = oracle.sgm_cost_volume(a, b, M, t, depths)
            sgm = (adaptive_ref.aggregate(cost, a, 6, 96, literal=False) if adaptive
                   else oracle.sgm_aggregate(cost, 6, 96))
            plane, argmin = oracle.sgm_depth_from_volume(sgm, a, depths)
            return (subplane_ref.subplane_depth(sgm, argmin, a, rng[0], rng[1]) if subplane
                    else plane)
        maps = []
        for nb in nbs:
            fwd = run(main, nb["image"], nb["M_fwd"], nb["t_fwd"], nb["range_main"])
            bwd = run(nb["image"], main, nb["M_bwd"], nb["t_bwd"], nb["range_neighbor"])
            maps.append(oracle.sgm_lr_check(fwd, bwd, nb["M_fwd"], nb["t_fwd"]))
        stack = np.stack(maps)
        stack.setflags(write=False)
        _CHECKED[key] = stack
    return _CHECKED[key]


def _view_opts_entry(main, nbs, D, adaptive, subplane):
    """smvs_sgm_depth_for_view_opts itself, whatever device.sgm_depth_for_view
    goes through"""
    from smvs_amd import _capi, device
    lib = _capi.load()
    keep = []
    arr = device._sgm_neighbors(nbs, keep)
    h, w = main.shape
    depth = np.zeros((h, w), F)
    opts = device.SgmOptions(1 if adaptive else 0, 1 if subplane else 0)
    main = np.ascontiguousarray(main, np.uint8)
    rc = lib.smvs_sgm_depth_for_view_opts(0, main.ctypes.data_as(C.POINTER(C.c_uint8)), w, h, arr,
                                          len(nbs), D, C.c_uint16(6), C.c_uint16(96),
                                          C.byref(opts), depth.ctypes.data_as(C.POINTER(C.c_float)))
    assert rc == 0, lib.smvs_last_error()
    return depth


def _view_merge_entry(main, nbs, D, adaptive, subplane, merge, min_agree, ratio):
    """smvs_sgm_depth_for_view_merge itself (no optional outputs)"""
    from smvs_amd import _capi, device
    lib = _capi.load()
    keep = []
    arr = device._sgm_neighbors(nbs, keep)
    h, w = main.shape
    depth = np.zeros((h, w), F)
    opts = device.SgmViewOptions(1 if adaptive else 0, 1 if subplane else 0, merge, min_agree,
                                 ratio)
    main = np.ascontiguousarray(main, np.uint8)
    rc = lib.smvs_sgm_depth_for_view_merge(0, main.ctypes.data_as(C.POINTER(C.c_uint8)), w, h,
                                           arr, len(nbs), D, C.c_uint16(6), C.c_uint16(96),
                                           C.byref(opts), depth.ctypes.data_as(C.POINTER(C.c_float)),
                                           None, None)
    assert rc == 0, lib.smvs_last_error()
    return depth


MODES = [(False, False), (True, True)]


@pytest.mark.parametrize("adaptive,subplane", MODES, ids=["constant", "adaptive-subplane"])
def test_view_front_end_over_four_neighbours(hip, oracle, scene_inputs, adaptive, subplane):
    """6. device.sgm_depth_for_view(consensus=True) on SGM-scale images and, with
    halvings=1, on raw images == the forward and backward runs of the oracle
    (the restatements' in the adaptive, sub-plane mode), oracle.sgm_lr_check, the
    consensus restatement at (0.95, 2); the checked maps and the support of
    want_checked are the composition's; with two neighbours the reference's
    merge, and the consensus at (0, 1), have the bytes of the `_opts` entry.

    Counted on the CPU on this scene, constant mode, 64 planes: pixels by
    number of valid checked maps 734 / 1395 / 3420 / 3476 / 15551 for 0 .. 4;
    best-star sizes 734 / 1823 / 3416 / 3420 / 15183; winner not the first
    valid map at 283 pixels; a valid map outside the star at 1094; 89.6 %
    valid at min_agree 2."""
    main, nbs = _front_end_inputs(scene_inputs)
    assert main.shape == (128, 192) and len(nbs) == 4
    stack = _checked_maps(oracle, scene_inputs, adaptive, subplane)
    merged, support, best = ref.consensus(stack, 0.95, 2)
    valid = stack != 0
    by_valid = np.bincount(valid.sum(axis=0).ravel(), minlength=5)
    by_star = np.bincount(support.ravel(), minlength=5)
    c = branch_counts(stack, 0.95, 2)
    print("valid maps 0..4: %s; best-star sizes 0..4: %s; %s; %.1f %% valid"
          % (list(by_valid), list(by_star), c, 100.0 * (merged != 0).mean()))
    assert np.all(by_valid >= 1) and np.all(by_star >= 1)
    for key in ("winner_not_first", "valid_outside_star", "min_agree_rejects", "full_support",
                "merged_valid"):
        assert c[key] >= 1, key

    got = hip.sgm_depth_for_view(main, nbs, num_steps=PLANES, adaptive_p2=adaptive,
                                 subplane=subplane, consensus=True, want_checked=True)
    assert np.array_equal(got["checked"], stack)
    assert np.array_equal(got["support"], support)
    assert np.array_equal(got["depth"], merged)
    lean = hip.sgm_depth_for_view(main, nbs, num_steps=PLANES, adaptive_p2=adaptive,
                                  subplane=subplane, consensus=True)
    assert np.array_equal(lean, merged)
    raw = [dict(nb, image=scene_inputs["images"][k + 1]) for k, nb in enumerate(nbs)]
    got = hip.sgm_depth_for_view(scene_inputs["images"][0], raw, num_steps=PLANES,
                                 adaptive_p2=adaptive, subplane=subplane, halvings=1,
                                 consensus=True, want_checked=True)
    assert np.array_equal(got["checked"], stack)
    assert np.array_equal(got["support"], support)
    assert np.array_equal(got["depth"], merged)
    # other parameters: everything valid anywhere, and full agreement only
    for ratio, min_agree in ((0.0, 1), (1.0, 4), (0.8, 3)):
        want = ref.consensus(stack, ratio, min_agree)[0]
        assert np.array_equal(hip.sgm_depth_for_view(
            main, nbs, num_steps=PLANES, adaptive_p2=adaptive, subplane=subplane, consensus=True,
            agree_ratio=ratio, min_agree=min_agree), want), (ratio, min_agree)

    # two neighbours: the reference's merge through the new entry and the
    # consensus at (0, 1) have the `_opts` entry's bytes
    two = _view_opts_entry(main, nbs[:2], PLANES, adaptive, subplane)
    assert np.array_equal(two, ref.reference_merge(stack[0], stack[1]))
    assert (two != 0).mean() > 0.5
    assert _view_merge_entry(main, nbs[:2], PLANES, adaptive, subplane, 0, 0, 0.0).tobytes() \
        == two.tobytes()
    assert _view_merge_entry(main, nbs[:2], PLANES, adaptive, subplane, 1, 1, 0.0).tobytes() \
        == two.tobytes()
    assert hip.sgm_depth_for_view(main, nbs[:2], num_steps=PLANES, adaptive_p2=adaptive,
                                  subplane=subplane).tobytes() == two.tobytes()
    # one neighbour, min_agree 1: the checked map itself
    one = hip.sgm_depth_for_view(main, nbs[:1], num_steps=PLANES, adaptive_p2=adaptive,
                                 subplane=subplane, consensus=True, min_agree=1)
    assert np.array_equal(one, stack[0])


def test_host_mirror_over_four_neighbours(hip, oracle, scene_inputs):
    """7. host.sgm_depth(neighbors=4, consensus=True) is the map of test 6; the
    default call is oracle.sgm_depth_for_view, as before."""
    from smvs_amd import host
    stack = _checked_maps(oracle, scene_inputs, False, False)
    want = ref.consensus(stack, 0.95, 2)[0]
    got = host.sgm_depth(scene_inputs, 1, num_steps=PLANES, neighbors=4, consensus=True)
    assert np.array_equal(got, want)
    # fewer neighbours asked for than there are: the first three
    assert np.array_equal(host.sgm_depth(scene_inputs, 1, num_steps=PLANES, neighbors=3,
                                         consensus=True, agree_ratio=0.8, min_agree=1),
                          ref.consensus(stack[:3], 0.8, 1)[0])
    # more asked for than there are: capped by the neighbours the view has
    assert np.array_equal(host.sgm_depth(scene_inputs, 1, num_steps=PLANES, neighbors=6,
                                         consensus=True), want)
    assert np.array_equal(host.sgm_depth(scene_inputs, 1),
                          oracle.sgm_depth_for_view(scene_inputs, sgm_scale=1))
    assert np.array_equal(host.sgm_depth(scene_inputs, 1, num_steps=PLANES),
                          ref.reference_merge(stack[0], stack[1]))


def _rel(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b) / max(np.linalg.norm(b), 1e-300))


def test_optimize_from_the_consensus_map_matches_oracle(hip, oracle, scene_inputs):
    """8. DepthOptimizer::optimize started from the consensus map: C++ host + HIP
    against the oracle's optimiser started from the same map.  The units and
    bounds of the sub-plane case (tests/test_gpu_sgm_subplane.py): batch log in
    the bench metric's units (tests/parity_units.py, no drift allowance), the
    valid pixels identical, depth within 1e-4 relative L2."""
    from smvs_amd import host
    stack = _checked_maps(oracle, scene_inputs, False, False)
    want_map = ref.consensus(stack, 0.95, 2)[0]
    sgm = host.sgm_depth(scene_inputs, sgm_scale=1, num_steps=PLANES, neighbors=4,
                         consensus=True)
    assert np.array_equal(sgm, want_map)
    got = host.optimize(scene_inputs, regularization=0.01, num_iterations=5, min_scale=2,
                        sgm_depth=sgm)
    want = oracle.optimize(scene_inputs, regularization=0.01, num_iterations=5, min_scale=2,
                           sgm_depth=got["sgm_roundtrip"])
    assert_same_units(got["log"], want["log"], 384, 256, "sgm_consensus_384x256")
    assert np.array_equal(got["depth"] > 0, want["depth"] > 0)
    assert (want["depth"] > 0).mean() > 0.5
    print("depth rel L2 %.3e" % _rel(got["depth"], want["depth"]))
    assert _rel(got["depth"], want["depth"]) <= 1e-4


# --------------------------------------------------------------------- the scene
def _stored(inputs, z):
    """What write_depth_to_view stores for the z-depth map z as "smvs-sgm"
    (MVE's ray-length convention), through the unchanged host mirror
    (tests/test_gpu_sgm_wide.py)."""
    from smvs_amd import host
    host.optimize(inputs, regularization=0.01, num_iterations=1, min_scale=2, sgm_depth=z)
    return host.last_embeddings()["smvs-sgm"]


def _sgm_file(d):
    with open(os.path.join(d, "views", "view_0000.mve", "smvs-sgm.mvei"), "rb") as f:
        return f.read()


def _spread_ring_inputs():
    """The sphere scene of synth.pipeline_inputs with the four neighbours on
    rings of different radii.  (ViewSelection keeps one view per distance from
    the main view, as the reference's std::map does, view_selection.cc:134-159:
    of the equidistant ring of pipeline_inputs it selects two.)"""
    from smvs_amd import synth
    w, h, flen, seed = 384, 256, 1.2, 1234
    rng = np.random.default_rng(seed)
    main = synth.ring_cameras(w, h, N_NEIGHBORS, flen=flen)[0]
    subs = [synth.ring_cameras(w, h, N_NEIGHBORS, flen=flen, ring=0.28 - 0.02 * k)[1][k]
            for k in range(N_NEIGHBORS)]
    scene = synth.SphereScene(seed=seed, px_size=3.0 / (flen * max(w, h)))
    cams = [main] + subs
    images = [synth.render_rgb(scene, c, None) for c in cams]
    xs = rng.uniform(0.05 * w, 0.95 * w, 2000)
    ys = rng.uniform(0.05 * h, 0.95 * h, 2000)
    X, _ = scene.intersect(main.center, synth.pixel_rays(main, xs, ys))
    return dict(scene=scene, cams=cams, images=images, features=X.astype(np.float32),
                view_ids=list(range(len(cams))))


def test_reconstruct_scene_with_the_consensus(hip, oracle, tmp_path):
    """9. ReconSettings::sgm_neighbors / sgm_consensus: the smvs-sgm embedding of
    the scene run is the view-level front end for the four neighbours
    ViewSelection chose, in its order (not the order of the views); a default
    run writes the file the previous last entry of the chain
    (smvs_host_reconstruct_scene_subplane) writes."""
    from smvs_amd import host, mve_scene
    inputs = _spread_ring_inputs()
    scene = dict(views=[dict(id=i, flen=c.flen, rot=c.R, trans=c.t, width=384, height=256)
                        for i, c in enumerate(inputs["cams"])],
                 features=inputs["features"],
                 refs=[list(range(5))] * len(inputs["features"]))
    nb = host.select_neighbors(scene, 0, num_neighbors=4)
    assert sorted(nb) == [1, 2, 3, 4] and nb != [1, 2, 3, 4]
    order = [0] + nb
    sel = dict(inputs, cams=[inputs["cams"][i] for i in order],
               images=[inputs["images"][i] for i in order], view_ids=order)
    stack = _checked_maps(oracle, sel, False, False)
    want = ref.consensus(stack, 0.95, 2)[0]
    assert (want != 0).mean() > 0.5
    # (ties keep the lowest k: the neighbours' order shows in the map)
    assert not np.array_equal(want, ref.consensus(stack[np.argsort(nb)], 0.95, 2)[0])
    dirs = {}
    for name in ("consensus", "default", "old"):
        dirs[name] = str(tmp_path / name)
        os.makedirs(dirs[name])
        mve_scene.write_scene(dirs[name], inputs)
    done, skipped, _ = host.reconstruct_scene(dirs["consensus"], view_ids=[0], num_neighbors=4,
                                              min_neighbors=2, output_scale=2,
                                              sgm_num_steps=PLANES, sgm_neighbors=4,
                                              sgm_consensus=True)
    assert done == [0] and skipped == 0
    got = mve_scene.load_mvei(os.path.join(dirs["consensus"], "views", "view_0000.mve",
                                           "smvs-sgm.mvei"))
    assert got.shape == (128, 192)
    assert np.array_equal(got, _stored(sel, want))
    done, skipped, _ = host.reconstruct_scene(dirs["default"], view_ids=[0], num_neighbors=4,
                                              min_neighbors=2, output_scale=2)
    assert done == [0] and skipped == 0
    assert _sgm_file(dirs["default"]) != _sgm_file(dirs["consensus"])
    # the same settings through the previous last entry of the chain
    hlib = host.load()
    st = host.ReconSettings(b"undistorted", 1.0, 2, 0, 1, 0, 0, 0, 0.0, 0.0, 1, 4, 2, 0, 1, 2,
                            -1, 1700000)
    ids = np.array([0], np.int32)
    n = C.c_int(0)
    rc = hlib.smvs_host_reconstruct_scene_subplane(
        dirs["old"].encode(), C.byref(st), C.c_uint(0), C.c_int(128), C.c_int(0),
        ids.ctypes.data_as(C.POINTER(C.c_int32)), C.c_int(1), None, C.c_int(0), C.byref(n),
        None, None, None)
    assert rc == 0 and n.value == 1
    assert _sgm_file(dirs["old"]) == _sgm_file(dirs["default"])
