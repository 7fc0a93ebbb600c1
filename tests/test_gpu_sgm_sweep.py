"""GPU parity of the multi-neighbour plane sweep of the SGM front end (DESIGN.md
section 3.6, "plane sweep"; include/smvs_hip.h, "Multi-neighbour plane sweep"):
the fold kernel on random bytes against the numpy restatement
tests/sgm_sweep_ref.py, a view's sweep against the composition of the oracle's
pieces and the restatements (tests/sgm_sweep_compose.py), one neighbour against
smvs_sgm_run_opts, the raw entry, the host mirror, the scene run, the optimizer
started from the sweep map, the launch counts, and the entries that were there
before.  The definition is integers only: every comparison is array_equal."""
import ctypes as C
import os

import numpy as np
import pytest

import sgm_merge_ref as merge_ref       # tests/sgm_merge_ref.py
import sgm_sweep_compose as compose     # tests/sgm_sweep_compose.py
import sgm_sweep_ref as ref             # tests/sgm_sweep_ref.py
from parity_units import assert_same_units  # tests/parity_units.py

pytestmark = pytest.mark.gpu

F = np.float32
MODES = [(False, False), (True, True)]
MODE_IDS = ["constant", "adaptive-subplane"]


@pytest.fixture(scope="module")
def hip():
    import smvs_amd
    if smvs_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on a GPU")
    return smvs_amd


def defaults(n):
    """(min_views, best_k, support_cost, min_support) at n neighbours"""
    return min(2, n), (n + 1) // 2, 20, min(2, n)


# ------------------------------------------------------------ the fold kernel
LENGTHS = (70 * 37 * 30, 15, 16)     # no multiple of 16; a tail alone; one vector alone


def random_costs(n, length, seed):
    """bytes over 0 .. 255 with 255 at about a quarter of the positions"""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 256, (n, length)).astype(np.uint8)
    c[rng.random((n, length)) < 0.25] = 255
    return c


@pytest.mark.parametrize("n", [1, 2, 3, 6, 16])
def test_fold_kernel_on_random_bytes(hip, n):
    """1. smvs_sgm_fold_costs == the restatement for lengths 77,700 (no multiple
    of 16), 15 and 16, min_views in {1, 2, n}, best_k in {0, 1, (n + 1) / 2, n,
    16}; for n = 2 also on all 256 x 256 pairs of bytes."""
    inputs = [random_costs(n, length, 1000 * n + length % 97) for length in LENGTHS]
    assert abs((inputs[0] == 255).mean() - 0.25) < 0.01
    if n == 2:
        a, b = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
        inputs.append(np.stack([a.ravel(), b.ravel()]).astype(np.uint8))
    for costs in inputs:
        for min_views in sorted({1, min(2, n), n}):
            for best_k in sorted({0, 1, (n + 1) // 2, n, 16}):
                want = ref.fold(costs, min_views, best_k)
                got = hip.sgm_fold_costs(costs, min_views=min_views, best_k=best_k)
                assert got.dtype == np.uint8 and got.shape == want.shape
                assert np.array_equal(got, want), (costs.shape, min_views, best_k)


# -------------------------------------------------------------- a view's sweep
SIZES = [(70, 37), (64, 40), (33, 29)]      # (width, height) of the neighbours, cycled
RANGE = (2.0, 10.0)
_SCENES = {}
_VOLUMES = {}


def small_scene(w, h, n=6):
    """A w x h main view of the sphere scene and n ring neighbours of the SIZES,
    with the float reprojections main -> neighbour."""
    from smvs_amd import synth
    if (w, h, n) not in _SCENES:
        main, subs = synth.ring_cameras(w, h, n, flen=1.2)
        scene = synth.SphereScene(px_size=3.0 / (1.2 * 96))
        nbs = []
        for k, c in enumerate(subs):
            nw, nh = SIZES[k % len(SIZES)] if (w, h) == SIZES[0] else (w + 2 * (k % 3), h + (k % 2))
            cam = synth.Camera(c.R, c.t, c.flen, nw, nh)
            M, t = synth.reprojection(main, cam)
            nbs.append(dict(image=synth.render(scene, cam), M_fwd=M.astype(F).reshape(9),
                            t_fwd=t.astype(F).reshape(3)))
        _SCENES[(w, h, n)] = (synth.render(scene, main), nbs)
    return _SCENES[(w, h, n)]


def volumes(oracle, w, h, D):
    """the six neighbours' cost volumes over the main view's D planes, once"""
    if (w, h, D) not in _VOLUMES:
        main, nbs = small_scene(w, h)
        v = compose.neighbour_volumes(oracle, main, nbs, RANGE, D)
        v.setflags(write=False)
        _VOLUMES[(w, h, D)] = v
    return _VOLUMES[(w, h, D)]


def check_against_composition(hip, oracle, w, h, n, D, adaptive, subplane):
    main, nbs = small_scene(w, h)
    min_views, best_k, support_cost, min_support = defaults(n)
    want = compose.sweep(oracle, main, nbs[:n], RANGE, D, adaptive, subplane, min_views, best_k,
                         support_cost, min_support, vols=volumes(oracle, w, h, D)[:n])
    got = hip.sgm_sweep_for_view(main, nbs[:n], RANGE, num_steps=D, adaptive_p2=adaptive,
                                 subplane=subplane, want_volumes=True)
    assert np.array_equal(got["cost"], want["cost"])
    assert np.array_equal(got["sgm"], want["sgm"])
    assert np.array_equal(got["argmin"], want["argmin"])
    assert np.array_equal(got["support"], want["support"])
    assert np.array_equal(got["depth"], want["depth"])
    # without the volumes (another form of the path kernels where S is not asked for)
    lean = hip.sgm_sweep_for_view(main, nbs[:n], RANGE, num_steps=D, adaptive_p2=adaptive,
                                  subplane=subplane)
    assert np.array_equal(lean["depth"], want["depth"])
    assert np.array_equal(lean["argmin"], want["argmin"])
    assert np.array_equal(lean["support"], want["support"])
    return want


@pytest.mark.parametrize("adaptive,subplane", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("D", [16, 30, 136])
@pytest.mark.parametrize("n", [1, 3, 6])
def test_sweep_against_the_composition(hip, oracle, n, D, adaptive, subplane):
    """2. smvs_sgm_sweep_for_view on a 70 x 37 main view with neighbours of
    70 x 37, 64 x 40 and 33 x 29 == per neighbour oracle.sgm_cost_volume, the
    fold, the aggregation (oracle, or the adaptive restatement), the winners
    (oracle, or the sub-plane restatement), the support: depth, argmin, support,
    cost and sgm, at the defaults for n neighbours.  16 planes: the packed cost
    kernel; 30: the tiled one; 136: the wide path kernel."""
    w, h = SIZES[0]
    want = check_against_composition(hip, oracle, w, h, n, D, adaptive, subplane)
    if n == 6 and D == 30:
        # the test says something: depths, rejections by the support, folded
        # bytes that are no cost
        assert (want["depth"] != 0).mean() > 0.3
        assert ((want["unchecked"] != 0) & (want["depth"] == 0)).any()
        assert (want["cost"] == 255).any() and (want["cost"] != 255).any()


@pytest.mark.parametrize("adaptive,subplane", MODES, ids=MODE_IDS)
def test_sweep_on_the_smallest_image(hip, oracle, adaptive, subplane):
    """2. (cont.) the same at 11 x 9, the smallest image smvs_sgm_run takes"""
    check_against_composition(hip, oracle, 11, 9, 3, 16, adaptive, subplane)


@pytest.mark.parametrize("adaptive,subplane", MODES, ids=MODE_IDS)
def test_one_neighbour_is_the_run(hip, adaptive, subplane):
    """3. n = 1, min_views = 1, min_support = 0: depth, argmin, cost and sgm of
    smvs_sgm_run_opts on the same pair."""
    w, h = SIZES[0]
    main, nbs = small_scene(w, h)
    for D in (16, 30, 136):
        nb = nbs[1]
        run = hip.sgm_run(main, nb["image"], nb["M_fwd"], nb["t_fwd"], RANGE[0], RANGE[1], D,
                          want_volumes=True, adaptive_p2=adaptive, subplane=subplane)
        got = hip.sgm_sweep_for_view(main, [nb], RANGE, num_steps=D, adaptive_p2=adaptive,
                                     subplane=subplane, min_views=1, best_k=0, min_support=0,
                                     want_volumes=True)
        for key in ("depth", "argmin", "cost", "sgm"):
            assert np.array_equal(got[key], run[key]), (D, key)
        assert (run["depth"] != 0).mean() > 0.3


# ------------------------------------------------------ the 384 x 256 sphere scene
N_NEIGHBORS = 4
PLANES = 64


@pytest.fixture(scope="module")
def scene_inputs():
    from smvs_amd import synth
    return synth.pipeline_inputs("sphere", 384, 256, N_NEIGHBORS, flen=1.2)


_WANT = {}


def scene_composition(oracle, inputs, n=N_NEIGHBORS):
    """the sweep map of the scene's main view at the defaults for n neighbours"""
    key = (tuple(inputs["view_ids"]), n)
    if key not in _WANT:
        main, nbs, rng = compose.front_end_inputs(inputs, n)
        min_views, best_k, support_cost, min_support = defaults(n)
        got = compose.sweep(oracle, main, nbs, rng, PLANES, False, False, min_views, best_k,
                            support_cost, min_support)
        for a in got.values():
            a.setflags(write=False)
        _WANT[key] = got
    return _WANT[key]


def test_raw_entry(hip, scene_inputs):
    """4. smvs_sgm_sweep_for_view_raw with halvings = 1 on the 3-channel images ==
    the SGM-scale entry on host.sgm_image's outputs: depth and support."""
    main, nbs, rng = compose.front_end_inputs(scene_inputs, N_NEIGHBORS)
    assert main.shape == (128, 192) and scene_inputs["images"][0].shape == (256, 384, 3)
    want = hip.sgm_sweep_for_view(main, nbs, rng, num_steps=PLANES)
    raw = [dict(nb, image=scene_inputs["images"][k + 1]) for k, nb in enumerate(nbs)]
    got = hip.sgm_sweep_for_view(scene_inputs["images"][0], raw, rng, num_steps=PLANES,
                                 halvings=1)
    assert sorted(got) == ["depth", "support"]
    assert np.array_equal(got["depth"], want["depth"])
    assert np.array_equal(got["support"], want["support"])
    assert (want["depth"] != 0).mean() > 0.5 and want["support"].max() == N_NEIGHBORS


def test_host_mirror(hip, oracle, scene_inputs):
    """5. host.sgm_depth(neighbors=4, sweep=True) is the composition; other values
    of the options arrive; sweep together with consensus raises; the default
    call is oracle.sgm_depth_for_view, as before."""
    from smvs_amd import _capi, host
    want = scene_composition(oracle, scene_inputs)
    got = host.sgm_depth(scene_inputs, 1, num_steps=PLANES, neighbors=4, sweep=True)
    assert np.array_equal(got, want["depth"])
    assert (got != 0).mean() > 0.5
    assert ((want["unchecked"] != 0) & (want["depth"] == 0)).any()
    # more asked for than there are: capped by the neighbours the view has
    assert np.array_equal(host.sgm_depth(scene_inputs, 1, num_steps=PLANES, neighbors=6,
                                         sweep=True), want["depth"])
    main, nbs, rng = compose.front_end_inputs(scene_inputs, 3)
    other = compose.sweep(oracle, main, nbs, rng, PLANES, False, False, 3, 1, 7, 3,
                          vols=want["vols"][:3])
    assert np.array_equal(host.sgm_depth(scene_inputs, 1, num_steps=PLANES, neighbors=3,
                                         sweep=True, sweep_min_views=3, sweep_best_k=1,
                                         sweep_support_cost=7, sweep_min_support=3),
                          other["depth"])
    assert not np.array_equal(other["depth"], want["depth"])
    with pytest.raises(_capi.SmvsError) as e:
        host.sgm_depth(scene_inputs, 1, num_steps=PLANES, neighbors=4, sweep=True, consensus=True)
    assert "sweep" in str(e.value)
    assert np.array_equal(host.sgm_depth(scene_inputs, 1),
                          oracle.sgm_depth_for_view(scene_inputs, sgm_scale=1))


def _rel(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b) / max(np.linalg.norm(b), 1e-300))


def test_optimize_from_the_sweep_map_matches_oracle(hip, oracle, scene_inputs):
    """5. (cont.) DepthOptimizer::optimize started from the sweep map: C++ host +
    HIP against the oracle's optimiser started from the same map.  The units and
    bounds of the consensus case (tests/test_gpu_sgm_merge.py): batch log in the
    bench metric's units (tests/parity_units.py, no drift allowance), the valid
    pixels identical, depth within 1e-4 relative L2."""
    from smvs_amd import host
    want_map = scene_composition(oracle, scene_inputs)["depth"]
    sgm = host.sgm_depth(scene_inputs, sgm_scale=1, num_steps=PLANES, neighbors=4, sweep=True)
    assert np.array_equal(sgm, want_map)
    got = host.optimize(scene_inputs, regularization=0.01, num_iterations=5, min_scale=2,
                        sgm_depth=sgm)
    want = oracle.optimize(scene_inputs, regularization=0.01, num_iterations=5, min_scale=2,
                           sgm_depth=got["sgm_roundtrip"])
    assert_same_units(got["log"], want["log"], 384, 256, "sgm_sweep_384x256")
    assert np.array_equal(got["depth"] > 0, want["depth"] > 0)
    assert (want["depth"] > 0).mean() > 0.5
    print("depth rel L2 %.3e" % _rel(got["depth"], want["depth"]))
    assert _rel(got["depth"], want["depth"]) <= 1e-4


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
    rings of different radii: ViewSelection keeps one view per distance from the
    main view (tests/test_gpu_sgm_merge.py)."""
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


def test_reconstruct_scene_with_the_sweep(hip, oracle, tmp_path):
    """5. (cont.) ReconSettings::sgm_neighbors / sgm_sweep: the smvs-sgm embedding
    of the scene run is the sweep map for the four neighbours ViewSelection
    chose, in its order; a default run writes the file the entry before this one
    (smvs_host_reconstruct_scene_merge) writes."""
    from smvs_amd import host, mve_scene
    inputs = _spread_ring_inputs()
    scene = dict(views=[dict(id=i, flen=c.flen, rot=c.R, trans=c.t, width=384, height=256)
                        for i, c in enumerate(inputs["cams"])],
                 features=inputs["features"],
                 refs=[list(range(5))] * len(inputs["features"]))
    nb = host.select_neighbors(scene, 0, num_neighbors=4)
    assert sorted(nb) == [1, 2, 3, 4]
    order = [0] + nb
    sel = dict(inputs, cams=[inputs["cams"][i] for i in order],
               images=[inputs["images"][i] for i in order], view_ids=order)
    want = scene_composition(oracle, sel)["depth"]
    assert (want != 0).mean() > 0.5
    dirs = {}
    for name in ("sweep", "default", "old"):
        dirs[name] = str(tmp_path / name)
        os.makedirs(dirs[name])
        mve_scene.write_scene(dirs[name], inputs)
    done, skipped, _ = host.reconstruct_scene(dirs["sweep"], view_ids=[0], num_neighbors=4,
                                              min_neighbors=2, output_scale=2,
                                              sgm_num_steps=PLANES, sgm_neighbors=4,
                                              sgm_sweep=True)
    assert done == [0] and skipped == 0
    got = mve_scene.load_mvei(os.path.join(dirs["sweep"], "views", "view_0000.mve",
                                           "smvs-sgm.mvei"))
    assert got.shape == (128, 192)
    assert np.array_equal(got, _stored(sel, want))
    done, skipped, _ = host.reconstruct_scene(dirs["default"], view_ids=[0], num_neighbors=4,
                                              min_neighbors=2, output_scale=2)
    assert done == [0] and skipped == 0
    assert _sgm_file(dirs["default"]) != _sgm_file(dirs["sweep"])
    hlib = host.load()
    st = host.ReconSettings(b"undistorted", 1.0, 2, 0, 1, 0, 0, 0, 0.0, 0.0, 1, 4, 2, 0, 1, 2,
                            -1, 1700000)
    ids = np.array([0], np.int32)
    n = C.c_int(0)
    rc = hlib.smvs_host_reconstruct_scene_merge(
        dirs["old"].encode(), C.byref(st), C.c_uint(0), C.c_int(128), C.c_int(0), C.c_int(2),
        C.c_int(0), C.c_float(0.95), C.c_int(2), ids.ctypes.data_as(C.POINTER(C.c_int32)),
        C.c_int(1), None, C.c_int(0), C.byref(n), None, None, None)
    assert rc == 0 and n.value == 1
    assert _sgm_file(dirs["old"]) == _sgm_file(dirs["default"])


# ------------------------------------------------------------------ the launches
K_NAMES = ["census", "warp", "cost", "paths", "wta", "lr_check", "merge", "bilateral"]


def _launches(lib, fn):
    """the launches per kernel class of one call of fn (after a warm-up call)"""
    fn()
    lib.smvs_sgm_profile(1, None, None)
    try:
        fn()
    finally:
        cnt = (C.c_longlong * 8)()
        lib.smvs_sgm_profile(0, None, cnt)
    return dict(zip(K_NAMES, [int(c) for c in cnt]))


@pytest.mark.parametrize("adaptive,subplane", MODES, ids=MODE_IDS)
def test_launch_counts(hip, adaptive, subplane):
    """6. One sweep call at n = 4: one census, four warps, four costs, one WTA,
    one fold (counted as merge), one support kernel (counted as lr_check), and as
    many path launches as one smvs_sgm_run_opts at the same size and options."""
    from smvs_amd import _capi
    lib = _capi.load()
    w, h = SIZES[0]
    main, nbs = small_scene(w, h)
    for D in (30, 136):
        sweep = _launches(lib, lambda: hip.sgm_sweep_for_view(
            main, nbs[:4], RANGE, num_steps=D, adaptive_p2=adaptive, subplane=subplane))
        run = _launches(lib, lambda: hip.sgm_run(
            main, nbs[0]["image"], nbs[0]["M_fwd"], nbs[0]["t_fwd"], RANGE[0], RANGE[1], D,
            adaptive_p2=adaptive, subplane=subplane))
        assert run["paths"] >= 1
        assert sweep == dict(census=1, warp=4, cost=4, paths=run["paths"], wta=1, lr_check=1,
                             merge=1, bilateral=0), D


# ------------------------------------------------------------------ defaults off
def test_other_entries_keep_their_bytes_around_a_sweep(hip, scene_inputs):
    """7. The reference's two-neighbour front end and the consensus front end, each
    run before and after a sweep call on the same workspace, return identical
    bytes (the sweep shares their buffers and leaves nothing behind in them)."""
    from smvs_amd import host
    imgs = [host.sgm_image(scene_inputs, k, 1) for k in range(N_NEIGHBORS + 1)]
    small = dict(scene_inputs, images=imgs)
    nbs = []
    for k in range(1, N_NEIGHBORS + 1):
        Mf, tf = host.view_reprojection(small, 0, k)
        Mb, tb = host.view_reprojection(small, k, 0)
        nbs.append(dict(image=imgs[k], M_fwd=Mf, t_fwd=tf, M_bwd=Mb, t_bwd=tb,
                        range_main=host.depth_range(scene_inputs, 0),
                        range_neighbor=host.depth_range(scene_inputs, k)))

    def reference():
        return hip.sgm_depth_for_view(imgs[0], nbs[:2], num_steps=PLANES)

    def consensus():
        return hip.sgm_depth_for_view(imgs[0], nbs, num_steps=PLANES, consensus=True,
                                      want_checked=True)

    def sweep():
        return hip.sgm_sweep_for_view(imgs[0], nbs, nbs[0]["range_main"], num_steps=PLANES)
    ref_before, con_before, sweep_before = reference(), consensus(), sweep()
    ref_after, con_after, sweep_after = reference(), consensus(), sweep()
    assert ref_before.tobytes() == ref_after.tobytes()
    for key in ("depth", "checked", "support"):
        assert con_before[key].tobytes() == con_after[key].tobytes(), key
    for key in ("depth", "argmin", "support"):
        assert sweep_before[key].tobytes() == sweep_after[key].tobytes(), key
    assert (ref_before != 0).mean() > 0.5 and (con_before["depth"] != 0).mean() > 0.5
    # the two-neighbour merge of the checked maps is still the reference's
    assert np.array_equal(ref_before, merge_ref.reference_merge(con_before["checked"][0],
                                                                con_before["checked"][1]))
