"""GPU parity of the two opt-in filters of the SGM front end (DESIGN.md section
3.6, "uniqueness test and speckle removal"; include/smvs_hip.h, "Two single-run
rejections"): the uniqueness WTA kernels against the numpy restatement
tests/sgm_filter_ref.py on the oracle's S, the speckle kernels alone on synthetic
maps, the front ends against the composition of the pieces, and filters off
against the entries they extend.  Both definitions fix every operation: every
comparison of a map is array_equal."""
import ctypes as C

import numpy as np
import pytest

import sgm_adaptive_ref as adaptive_ref  # tests/sgm_adaptive_ref.py
import sgm_filter_ref as ref             # tests/sgm_filter_ref.py
import sgm_merge_ref as merge_ref        # tests/sgm_merge_ref.py
import sgm_subplane_ref as subplane_ref  # tests/sgm_subplane_ref.py
import sgm_sweep_compose as compose      # tests/sgm_sweep_compose.py
import sgm_sweep_ref as sweep_ref        # tests/sgm_sweep_ref.py

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def hip():
    import smvs_amd
    if smvs_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on a GPU")
    return smvs_amd


# ------------------------------------------------------------------ one run
@pytest.fixture(scope="module")
def pair():
    return subplane_ref.scene_pair()


_WANT = {}


def _want(oracle, pair, D, lo, hi, adaptive, p2=96):
    """cost, S and winners of the oracle (the adaptive restatement's S in that
    mode), the plane and the sub-plane map: once per run and mode."""
    key = (D, lo, hi, adaptive, p2)
    if key not in _WANT:
        main, nbr, M, t = pair
        depths = oracle.sgm_depths(lo, hi, D)
        ckey = (D, lo, hi)
        if ckey not in _WANT:
            _WANT[ckey] = oracle.sgm_cost_volume(main, nbr, M, t, depths)
        cost = _WANT[ckey]
        sgm = (adaptive_ref.aggregate(cost, main, 6, p2, literal=False) if adaptive
               else oracle.sgm_aggregate(cost, 6, p2))
        plane, argmin = oracle.sgm_depth_from_volume(sgm, main, depths)
        got = dict(cost=cost, sgm=sgm, argmin=argmin, plane=plane,
                   subplane=subplane_ref.subplane_depth(sgm, argmin, main, lo, hi))
        for a in got.values():
            a.setflags(write=False)
        _WANT[key] = got
    return _WANT[key]


RUNS = [(128, 3, 12), (256, 1, 12), (200, 1, 12), (33, 1, 12), (8, 3, 12), (3, 3, 12)]
WINDOWS = (1, 4, 16)
UNIQUENESS = (10, 99)


def _counts(want, uniq, window):
    """where the comparison could pass emptily: over the oracle's valid pixels"""
    S, i = want["sgm"], want["argmin"].astype(np.int64)
    v = want["plane"] > 0
    rejected, runner, none = ref.uniqueness(S, i, uniq, window)
    b = np.take_along_axis(S.astype(np.int64), i[:, :, None], axis=2)[:, :, 0]
    pos = ref.runner_up_plane(S, i, window)
    some = v & ~none
    return {"valid": int(v.sum()), "rejected": int((rejected & v).sum()),
            "at the bound": int((some & (runner.astype(np.int64) * (100 - uniq) == b * 100)).sum()),
            "runner-up in the winner's group of four": int((some & (pos // 4 == i // 4)).sum()),
            "runner-up in another row of 16 lanes": int((some & (pos // 64 != i // 64)).sum()),
            "no competitor": int((v & none).sum())}


def _check_run(hip, pair, want, D, lo, hi, adaptive, subplane, p2=96):
    main, nbr, M, t = pair
    base = want["subplane"] if subplane else want["plane"]
    for window in WINDOWS:
        for uniq in UNIQUENESS:
            rejected, runner, _ = ref.uniqueness(want["sgm"], want["argmin"], uniq, window)
            depth = ref.apply_uniqueness(base, rejected)
            tag = (D, lo, hi, adaptive, subplane, window, uniq)
            # every volume: S is asked for
            full = hip.sgm_run(main, nbr, M, t, lo, hi, D, p2=p2, want_volumes=True,
                               adaptive_p2=adaptive, subplane=subplane, uniqueness=uniq,
                               uniqueness_window=window)
            assert np.array_equal(full["cost"], want["cost"]), tag
            assert np.array_equal(full["sgm"], want["sgm"]), tag
            assert np.array_equal(full["argmin"], want["argmin"]), tag
            assert full["runner_up"].dtype == np.uint16
            assert np.array_equal(full["runner_up"], runner), tag
            assert np.array_equal(full["depth"], depth), tag
            # depth and argmin alone: S only in registers where the plan allows
            lean = hip.sgm_run(main, nbr, M, t, lo, hi, D, p2=p2, adaptive_p2=adaptive,
                               subplane=subplane, uniqueness=uniq, uniqueness_window=window)
            assert "runner_up" not in lean
            assert np.array_equal(lean["argmin"], want["argmin"]), tag
            assert np.array_equal(lean["depth"], depth), tag


@pytest.mark.parametrize("adaptive", [False, True], ids=["constant", "adaptive"])
@pytest.mark.parametrize("subplane", [False, True], ids=["plane", "subplane"])
@pytest.mark.parametrize("D,lo,hi", RUNS, ids=["%d-%d-%d" % r for r in RUNS])
def test_run_matches_the_restatement(hip, oracle, pair, D, lo, hi, subplane, adaptive):
    """1. smvs_sgm_run_filtered at windows 1, 4, 16 and uniqueness 10, 99, with
    every volume and with depth and argmin alone: depth, argmin and runner_up are
    the restatement's on the oracle's S (the adaptive restatement's).  128, 256,
    200 and 8 planes take the kernels that form S in registers (32 or 64 lanes
    per pixel), 33 and 3 planes the kernel that reads S.

    Counted on the CPU over the oracle's valid pixels, constant mode, uniqueness
    10: (128, 3, 12) window 1: 3267 of 6106 rejected, 60 exactly at the bound,
    the runner-up in the winner's own group of four planes at 3448 and in another
    row of 16 lanes at 31; window 4: 1100, 8: 569, 16: 356 rejected;
    (256, 1, 12) window 1: 2028 rejected, another row of 16 lanes at 589;
    (33, 1, 12) window 1: 233 of 5156 rejected, window 16: 5 without a
    competitor; (8, 3, 12) window 4: 468 of 3915 without a competitor."""
    want = _want(oracle, pair, D, lo, hi, adaptive)
    if not adaptive:
        # the comparison does not pass emptily
        c1 = _counts(want, 10, 1)
        print("%s window 1: %s" % ((D, lo, hi), c1))
        assert c1["valid"] >= 1 and c1["rejected"] >= 1
        if (D, lo, hi) == (128, 3, 12):
            for key in ("at the bound", "runner-up in the winner's group of four",
                        "runner-up in another row of 16 lanes"):
                assert c1[key] >= 1, key
        if (D, lo, hi) == (256, 1, 12):
            assert c1["runner-up in another row of 16 lanes"] >= 1
        if (D, lo, hi) == (33, 1, 12):
            c16 = _counts(want, 10, 16)
            print("%s window 16: %s" % ((D, lo, hi), c16))
            assert c16["no competitor"] >= 1
        if (D, lo, hi) == (8, 3, 12):
            c4 = _counts(want, 10, 4)
            print("%s window 4: %s" % ((D, lo, hi), c4))
            assert c4["no competitor"] >= 1
    _check_run(hip, pair, want, D, lo, hi, adaptive, subplane)


@pytest.mark.parametrize("subplane", [False, True], ids=["plane", "subplane"])
def test_run_with_s_in_memory_at_128_planes(hip, oracle, pair, subplane):
    """1. (cont.) penalty2 = 300 does not fit the path bytes: 128 planes through
    the kernel that reads S, eight planes per lane."""
    want = _want(oracle, pair, 128, 3, 12, False, p2=300)
    assert _counts(want, 10, 1)["rejected"] >= 1
    _check_run(hip, pair, want, 128, 3, 12, False, subplane, p2=300)


# ------------------------------------------------------- the speckle kernels
SIZES = [(1, 1), (1, 257), (257, 1), (17, 15), (33, 31), (64, 64), (65, 63), (129, 65),
         (97, 67), (300, 300)]
PATTERNS = ["random", "serpentine", "equal", "checkerboard", "stripes-x", "stripes-y"]
SPECKLE_RATIO = 0.95


def pattern(name, w, h):
    """a (h, w) float map and the speckle_size to test it at"""
    y, x = np.mgrid[0:h, 0:w]
    if name == "random":
        # four levels, neighbouring ones inside the ratio, 30 % not valid (zeros,
        # negatives and NaNs among them)
        rng = np.random.default_rng(1000 * w + h)
        a = np.array([1.0, 1.03, 1.06, 2.0], F)[rng.integers(0, 4, (h, w))]
        bad = rng.random((h, w)) < 0.3
        a[bad] = np.array([0.0, -1.0, np.nan], F)[rng.integers(0, 3, int(bad.sum()))]
        return a, 4
    if name == "serpentine":
        # full even rows joined by one pixel at alternating ends of the odd rows,
        # depth rising slowly along the path: one component, the longest chain
        a = np.zeros((h, w), F)
        step = np.where((y // 2) % 2 == 0, x, w - 1 - x) + (y // 2) * (w + 1)
        a[0::2] = (1.0 + 1e-5 * step[0::2]).astype(F)
        odd = np.arange(1, h, 2)
        ends = np.where((odd // 2) % 2 == 0, w - 1, 0)
        a[odd, ends] = (1.0 + 1e-5 * ((odd // 2) * (w + 1) + w)).astype(F)
        return a, int((a > 0).sum())
    if name == "equal":
        return np.full((h, w), 2.5, F), w * h
    if name == "checkerboard":
        return np.where((x + y) % 2 == 0, F(1.0), F(3.0)).astype(F), 2
    if name == "stripes-x":
        return np.where(x % 2 == 0, F(1.0), F(3.0)).astype(F), max(h, 2)
    if name == "stripes-y":
        return np.where(y % 2 == 0, F(1.0), F(3.0)).astype(F), max(w, 2)
    raise ValueError(name)


_SPECKLE_WANT = {}


def speckle_want(name, w, h):
    """the restatement's sizes of a pattern, once"""
    if (name, w, h) not in _SPECKLE_WANT:
        a, k = pattern(name, w, h)
        size = ref.component_sizes(a, SPECKLE_RATIO)
        a.setflags(write=False)
        size.setflags(write=False)
        _SPECKLE_WANT[(name, w, h)] = (a, k, size)
    return _SPECKLE_WANT[(name, w, h)]


@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("w,h", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_speckle_kernels_on_synthetic_maps(hip, w, h, name):
    """2. smvs_sgm_filter_speckles == the restatement (a plain union-find over the
    link edges): out and size, at a size that removes some components and keeps
    others where the pattern has both, and one above it that removes all."""
    a, k, size = speckle_want(name, w, h)
    valid = a > 0
    if name == "serpentine":
        assert size[valid].min() == int(valid.sum())      # one component
    if name == "equal":
        assert (size == w * h).all()
    if name == "checkerboard" and w * h > 1:
        assert (size == 1).all()
    for speckle_size in (k, k + 1, 0):
        want = a.copy()
        want[(size > 0) & (size < speckle_size)] = 0
        out, got_size = hip.sgm_filter_speckles(a, speckle_size, SPECKLE_RATIO)
        assert got_size.dtype == np.uint32 and np.array_equal(got_size, size), speckle_size
        assert out.tobytes() == want.tobytes(), speckle_size
    if name == "random" and w * h >= 255:
        kept = (size >= 4).sum()
        assert 0 < kept < valid.sum()                     # some kept, some removed
        assert np.isnan(a).any() and (a < 0).any()


def test_speckle_entry_in_place_and_without_size(hip):
    """2. (cont.) out may be the input itself and size may be NULL."""
    from smvs_amd import _capi
    lib = _capi.load()
    a, k, size = speckle_want("random", 97, 67)
    want, _ = ref.filter_speckles(a, k, SPECKLE_RATIO)
    buf = a.copy()
    fp = buf.ctypes.data_as(C.POINTER(C.c_float))
    rc = lib.smvs_sgm_filter_speckles(0, fp, 97, 67, k, C.c_float(SPECKLE_RATIO), fp, None)
    assert rc == 0, lib.smvs_last_error()
    assert buf.tobytes() == want.tobytes()
    assert (want != a)[a > 0].any()


def test_speckle_kernels_on_pixels_that_are_not_valid(hip):
    """2. (cont.) A NaN with a payload, a negative, a zero and a negative zero are
    in no component and keep their bits; an infinite depth is valid and links
    with nothing at ratio 0.5; exact quotients at the ratio link."""
    a = np.array([[1.0, 0.0, 1.0, -2.0, 1.0, 0.0, 1.0, -0.0, 1.0, np.inf, np.inf, 0.0,
                   1.0, 0.5, 0.25, np.nextafter(F(0.125), F(0))]], F)
    a.view(np.uint32)[0, 1] = 0x7FC12345
    for shape in ((1, 16), (16, 1), (4, 4)):
        m = a.reshape(shape)
        for speckle_size in (2, 3, 4):
            want, size = ref.filter_speckles(m, speckle_size, 0.5)
            out, got_size = hip.sgm_filter_speckles(m, speckle_size, 0.5)
            assert np.array_equal(got_size, size), (shape, speckle_size)
            assert out.tobytes() == want.tobytes(), (shape, speckle_size)
    size = ref.component_sizes(a, 0.5)
    assert size.tolist() == [[1, 0, 1, 0, 1, 0, 1, 0, 1, 1, 1, 0, 3, 3, 3, 1]]


# ------------------------------------------------------------ the front ends
N_NEIGHBORS = 3
PLANES = 64
FILTER = dict(uniqueness=10, uniqueness_window=4, speckle_size=50, speckle_ratio=0.95)


@pytest.fixture(scope="module")
def scene_inputs():
    from smvs_amd import synth
    return synth.pipeline_inputs("sphere", 384, 256, N_NEIGHBORS, flen=1.2)


def _front_end_inputs(inputs, n=N_NEIGHBORS):
    """images, reprojections and depth ranges at SGM scale
    (tests/test_gpu_sgm_merge.py)"""
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


def _checked_maps(oracle, inputs, uniq, window, D=PLANES, n=N_NEIGHBORS):
    """The n checked forward maps of the view with the uniqueness test in all 2 n
    runs: oracle cost volume, aggregation and winners, the restatement's
    rejection, oracle.sgm_lr_check.  Also the rejections of the forward runs."""
    key = (tuple(inputs["view_ids"]), uniq, window, D, n)
    if key not in _CHECKED:
        main, nbs = _front_end_inputs(inputs, n)

        def run(a, b, M, t, rng):
            depths = oracle.sgm_depths(rng[0], rng[1], D)
            cost = oracle.sgm_cost_volume(a, b, M, t, depths)
            sgm = oracle.sgm_aggregate(cost, 6, 96)
            plane, argmin = oracle.sgm_depth_from_volume(sgm, a, depths)
            if uniq == 0:
                return plane, 0
            rejected = ref.uniqueness(sgm, argmin, uniq, window)[0]
            return ref.apply_uniqueness(plane, rejected), int((rejected & (plane > 0)).sum())
        maps, dropped = [], 0
        for nb in nbs:
            fwd, nf = run(main, nb["image"], nb["M_fwd"], nb["t_fwd"], nb["range_main"])
            bwd, nb_ = run(nb["image"], main, nb["M_bwd"], nb["t_bwd"], nb["range_neighbor"])
            dropped += nf + nb_
            maps.append(oracle.sgm_lr_check(fwd, bwd, nb["M_fwd"], nb["t_fwd"]))
        stack = np.stack(maps)
        stack.setflags(write=False)
        _CHECKED[key] = (stack, dropped)
    return _CHECKED[key]


def test_reference_merge_with_the_filters(hip, oracle, scene_inputs):
    """3. The reference's merge at n = 2 with both filters, SGM-scale and raw
    entry == the runs with the restatement's rejection, oracle.sgm_lr_check, the
    merge restatement, the speckle restatement; each filter alone too."""
    main, nbs = _front_end_inputs(scene_inputs)
    stack, dropped = _checked_maps(oracle, scene_inputs, 10, 4)
    plain, _ = _checked_maps(oracle, scene_inputs, 0, 1)
    merged = merge_ref.reference_merge(stack[0], stack[1])
    want, size = ref.filter_speckles(merged, 50, 0.95)
    removed = int(((merged > 0) & (want == 0)).sum())
    print("rejected by uniqueness in the four runs: %d; removed as speckles: %d of %d"
          % (dropped, removed, int((merged > 0).sum())))
    assert dropped >= 1 and removed >= 1 and (want != 0).mean() > 0.3
    got = hip.sgm_depth_for_view(main, nbs[:2], num_steps=PLANES, **FILTER)
    assert np.array_equal(got, want)
    raw = [dict(nb, image=scene_inputs["images"][k + 1]) for k, nb in enumerate(nbs)]
    got = hip.sgm_depth_for_view(scene_inputs["images"][0], raw[:2], num_steps=PLANES,
                                 halvings=1, **FILTER)
    assert np.array_equal(got, want)
    # one filter at a time
    got = hip.sgm_depth_for_view(main, nbs[:2], num_steps=PLANES, uniqueness=10,
                                 uniqueness_window=4)
    assert np.array_equal(got, merged)
    plain_merged = merge_ref.reference_merge(plain[0], plain[1])
    got = hip.sgm_depth_for_view(main, nbs[:2], num_steps=PLANES, speckle_size=50)
    assert np.array_equal(got, ref.filter_speckles(plain_merged, 50, 0.95)[0])
    # one neighbour: no merge launch in front of the filter
    got = hip.sgm_depth_for_view(main, nbs[:1], num_steps=PLANES, **FILTER)
    assert np.array_equal(got, ref.filter_speckles(stack[0], 50, 0.95)[0])


def test_consensus_with_the_filters(hip, oracle, scene_inputs):
    """3. (cont.) The consensus at n = 3 with both filters, SGM-scale and raw:
    depth is the speckle restatement of the consensus restatement of the checked
    maps; checked and support are those of the merge."""
    main, nbs = _front_end_inputs(scene_inputs)
    stack, _ = _checked_maps(oracle, scene_inputs, 10, 4)
    merged, support, _ = merge_ref.consensus(stack, 0.95, 2)
    want = ref.filter_speckles(merged, 50, 0.95)[0]
    assert ((merged > 0) & (want == 0)).any() and (want != 0).mean() > 0.3
    got = hip.sgm_depth_for_view(main, nbs, num_steps=PLANES, consensus=True, want_checked=True,
                                 **FILTER)
    assert np.array_equal(got["checked"], stack)
    assert np.array_equal(got["support"], support)
    assert np.array_equal(got["depth"], want)
    raw = [dict(nb, image=scene_inputs["images"][k + 1]) for k, nb in enumerate(nbs)]
    got = hip.sgm_depth_for_view(scene_inputs["images"][0], raw, num_steps=PLANES, halvings=1,
                                 consensus=True, **FILTER)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("subplane", [False, True], ids=["plane", "subplane"])
def test_sweep_with_the_filters(hip, oracle, scene_inputs, subplane):
    """3. (cont.) The sweep at n = 3 with both filters, SGM-scale and raw: the
    composition of tests/sgm_sweep_compose.py with the uniqueness restatement in
    front of the support test and the speckle restatement behind it; runner_up
    with the volumes."""
    main, nbs, rng = compose.front_end_inputs(scene_inputs, N_NEIGHBORS)
    n = N_NEIGHBORS
    min_views, best_k, support_cost, min_support = min(2, n), (n + 1) // 2, 20, min(2, n)
    base = compose.sweep(oracle, main, nbs, rng, PLANES, False, subplane, min_views, best_k,
                         support_cost, min_support)
    rejected, runner, _ = ref.uniqueness(base["sgm"], base["argmin"], 10, 4)
    unique = ref.apply_uniqueness(base["unchecked"], rejected)
    supported = sweep_ref.apply_support(unique, base["support"], min_support)
    want = ref.filter_speckles(supported, 50, 0.95)[0]
    assert (rejected & (base["unchecked"] > 0)).any()
    assert ((supported > 0) & (want == 0)).any() and (want != 0).mean() > 0.3
    got = hip.sgm_sweep_for_view(main, nbs, rng, num_steps=PLANES, subplane=subplane,
                                 want_volumes=True, **FILTER)
    assert np.array_equal(got["cost"], base["cost"])
    assert np.array_equal(got["sgm"], base["sgm"])
    assert np.array_equal(got["argmin"], base["argmin"])
    assert np.array_equal(got["support"], base["support"])
    assert np.array_equal(got["runner_up"], runner)
    assert np.array_equal(got["depth"], want)
    lean = hip.sgm_sweep_for_view(main, nbs, rng, num_steps=PLANES, subplane=subplane, **FILTER)
    assert "runner_up" not in lean
    assert np.array_equal(lean["depth"], want)
    raw = [dict(nb, image=scene_inputs["images"][k + 1]) for k, nb in enumerate(nbs)]
    got = hip.sgm_sweep_for_view(scene_inputs["images"][0], raw, rng, num_steps=PLANES,
                                 subplane=subplane, halvings=1, **FILTER)
    assert np.array_equal(got["depth"], want)
    assert np.array_equal(got["support"], base["support"])


def test_host_mirror_with_the_filters(hip, oracle, scene_inputs):
    """3. (cont.) host.sgm_depth with the four options is the composition for each
    of the three front ends; the default call is oracle.sgm_depth_for_view, as
    before."""
    from smvs_amd import host
    stack, _ = _checked_maps(oracle, scene_inputs, 10, 4)
    want = ref.filter_speckles(merge_ref.reference_merge(stack[0], stack[1]), 50, 0.95)[0]
    got = host.sgm_depth(scene_inputs, 1, num_steps=PLANES, **FILTER)
    assert np.array_equal(got, want) and (want != 0).mean() > 0.3
    want = ref.filter_speckles(merge_ref.consensus(stack, 0.95, 2)[0], 50, 0.95)[0]
    got = host.sgm_depth(scene_inputs, 1, num_steps=PLANES, neighbors=3, consensus=True,
                         **FILTER)
    assert np.array_equal(got, want)
    main, nbs, rng = compose.front_end_inputs(scene_inputs, N_NEIGHBORS)
    base = compose.sweep(oracle, main, nbs, rng, PLANES, False, False, 2, 2, 20, 2)
    rejected = ref.uniqueness(base["sgm"], base["argmin"], 10, 4)[0]
    supported = sweep_ref.apply_support(ref.apply_uniqueness(base["unchecked"], rejected),
                                        base["support"], 2)
    got = host.sgm_depth(scene_inputs, 1, num_steps=PLANES, neighbors=3, sweep=True, **FILTER)
    assert np.array_equal(got, ref.filter_speckles(supported, 50, 0.95)[0])
    # one option at a time arrives too
    plain, _ = _checked_maps(oracle, scene_inputs, 0, 1)
    merged = merge_ref.reference_merge(plain[0], plain[1])
    got = host.sgm_depth(scene_inputs, 1, num_steps=PLANES, speckle_size=50, speckle_ratio=0.9)
    assert np.array_equal(got, ref.filter_speckles(merged, 50, 0.9)[0])
    assert np.array_equal(host.sgm_depth(scene_inputs, 1, num_steps=PLANES), merged)


def _stored(inputs, z):
    """What write_depth_to_view stores for the z-depth map z as "smvs-sgm"
    (tests/test_gpu_sgm_sweep.py)."""
    from smvs_amd import host
    host.optimize(inputs, regularization=0.01, num_iterations=1, min_scale=2, sgm_depth=z)
    return host.last_embeddings()["smvs-sgm"]


def _spread_ring_inputs(n=3):
    """The sphere scene of synth.pipeline_inputs with the neighbours on rings of
    different radii: ViewSelection keeps one view per distance from the main view
    (tests/test_gpu_sgm_merge.py)."""
    from smvs_amd import synth
    w, h, flen, seed = 384, 256, 1.2, 1234
    rng = np.random.default_rng(seed)
    main = synth.ring_cameras(w, h, n, flen=flen)[0]
    subs = [synth.ring_cameras(w, h, n, flen=flen, ring=0.28 - 0.02 * k)[1][k] for k in range(n)]
    scene = synth.SphereScene(seed=seed, px_size=3.0 / (flen * max(w, h)))
    cams = [main] + subs
    images = [synth.render_rgb(scene, c, None) for c in cams]
    xs = rng.uniform(0.05 * w, 0.95 * w, 2000)
    ys = rng.uniform(0.05 * h, 0.95 * h, 2000)
    X, _ = scene.intersect(main.center, synth.pixel_rays(main, xs, ys))
    return dict(scene=scene, cams=cams, images=images, features=X.astype(np.float32),
                view_ids=list(range(len(cams))))


def test_reconstruct_scene_with_the_filters(hip, oracle, tmp_path):
    """3. (cont.) ReconSettings::sgm_uniqueness / sgm_uniqueness_window /
    sgm_speckle_size / sgm_speckle_ratio: the smvs-sgm embedding of a scene run
    is the filtered map of the reference's merge over the two neighbours
    ViewSelection chose first; a default run writes another file."""
    import os
    from smvs_amd import host, mve_scene
    inputs = _spread_ring_inputs()
    scene = dict(views=[dict(id=i, flen=c.flen, rot=c.R, trans=c.t, width=384, height=256)
                        for i, c in enumerate(inputs["cams"])],
                 features=inputs["features"],
                 refs=[list(range(4))] * len(inputs["features"]))
    nb = host.select_neighbors(scene, 0, num_neighbors=3)
    assert sorted(nb) == [1, 2, 3]
    order = [0] + nb
    sel = dict(inputs, cams=[inputs["cams"][i] for i in order],
               images=[inputs["images"][i] for i in order], view_ids=order)
    stack, _ = _checked_maps(oracle, sel, 10, 4, n=2)
    want = ref.filter_speckles(merge_ref.reference_merge(stack[0], stack[1]), 50, 0.95)[0]
    assert (want != 0).mean() > 0.3
    dirs = {}
    for name in ("filtered", "default"):
        dirs[name] = str(tmp_path / name)
        os.makedirs(dirs[name])
        mve_scene.write_scene(dirs[name], inputs)
    done, skipped, _ = host.reconstruct_scene(
        dirs["filtered"], view_ids=[0], num_neighbors=3, min_neighbors=2, output_scale=2,
        sgm_num_steps=PLANES, sgm_uniqueness=10, sgm_uniqueness_window=4, sgm_speckle_size=50,
        sgm_speckle_ratio=0.95)
    assert done == [0] and skipped == 0
    path = os.path.join("views", "view_0000.mve", "smvs-sgm.mvei")
    got = mve_scene.load_mvei(os.path.join(dirs["filtered"], path))
    assert got.shape == (128, 192)
    assert np.array_equal(got, _stored(sel, want))
    done, skipped, _ = host.reconstruct_scene(dirs["default"], view_ids=[0], num_neighbors=3,
                                              min_neighbors=2, output_scale=2,
                                              sgm_num_steps=PLANES)
    assert done == [0] and skipped == 0
    with open(os.path.join(dirs["default"], path), "rb") as f, \
            open(os.path.join(dirs["filtered"], path), "rb") as g:
        assert f.read() != g.read()


# ------------------------------------------------------------------ off is off
K_NAMES = ["census", "warp", "cost", "paths", "wta", "lr_check", "merge", "bilateral"]
OFF = [(0, 1, 0, 0.95), (0, 256, 1, 0.0), (0, 7, 0, 1.0)]


def _launches(lib, fn):
    """(result, launches per kernel class) of one call of fn after a warm-up"""
    fn()
    lib.smvs_sgm_profile(1, None, None)
    try:
        out = fn()
    finally:
        cnt = (C.c_longlong * 8)()
        lib.smvs_sgm_profile(0, None, cnt)
    return out, dict(zip(K_NAMES, [int(c) for c in cnt]))


def _same(a, b):
    if isinstance(a, dict):
        assert sorted(a) == sorted(b)
        for key in a:
            if a[key] is None:
                assert b[key] is None
            else:
                assert a[key].tobytes() == b[key].tobytes(), key
    else:
        assert a.tobytes() == b.tobytes()


def test_filters_off_are_the_parent_entries(hip, pair, scene_inputs):
    """4. Every `_filtered` entry with { 0, any window, 0 or 1, any ratio } gives
    the bytes and the launch counts of the entry it extends; the filters on add
    nothing but the speckle launches (class merge) and keep one WTA per run."""
    from smvs_amd import _capi, device
    lib = _capi.load()
    main, nbr, M, t = pair
    vmain, nbs = _front_end_inputs(scene_inputs)
    raw = [dict(nb, image=scene_inputs["images"][k + 1]) for k, nb in enumerate(nbs)]
    rng = nbs[0]["range_main"]

    def entries(**kw):
        return [
            lambda: hip.sgm_run(main, nbr, M, t, 3, 12, 128, want_volumes=True, **{
                k: v for k, v in kw.items() if k.startswith("uniq")}),
            lambda: hip.sgm_depth_for_view(vmain, nbs[:2], num_steps=PLANES, **kw),
            lambda: hip.sgm_depth_for_view(vmain, nbs, num_steps=PLANES, consensus=True,
                                           want_checked=True, **kw),
            lambda: hip.sgm_depth_for_view(scene_inputs["images"][0], raw[:2], num_steps=PLANES,
                                           halvings=1, **kw),
            lambda: hip.sgm_sweep_for_view(vmain, nbs, rng, num_steps=PLANES, want_volumes=True,
                                           **kw),
            lambda: hip.sgm_sweep_for_view(scene_inputs["images"][0], raw, rng, num_steps=PLANES,
                                           halvings=1, **kw)]
    parents = [_launches(lib, fn) for fn in entries()]
    for uniq, window, size, ratio in OFF:
        kw = dict(uniqueness=uniq, uniqueness_window=window, speckle_size=size,
                  speckle_ratio=ratio)
        # (the Python fronts call the entries without the filters at the defaults)
        assert (device._sgm_filter(uniq, window, size, ratio) is None) \
            == ((uniq, window, size, ratio) == OFF[0])
        for k, fn in enumerate(entries(**kw)):
            out, cnt = _launches(lib, fn)
            _same(out, parents[k][0])
            assert cnt == parents[k][1], (k, kw)
    # the defaults through the filtered entries themselves
    filt = device.SgmFilterOptions(*OFF[0])
    vopts = device._sgm_view_options(False, False, False, 0.95, 2)
    out, cnt = _launches(lib, lambda: device._sgm_depth_for_view_merge(
        lib, vmain, nbs[:2], PLANES, 6, 96, 0, vopts, None, False, filt))
    _same(out, parents[1][0])
    assert cnt == parents[1][1]
    # on: the same launches plus the speckle kernels (four; 192 x 128 is 24 tiles)
    on = dict(FILTER)
    for k in (1, 2, 4):
        _, cnt = _launches(lib, entries(**on)[k])
        want = dict(parents[k][1])
        want["merge"] += 4
        assert cnt == want, k


def test_existing_entries_keep_their_bytes_around_a_filtered_call(hip, scene_inputs):
    """4. (cont.) The reference front end, the consensus and the sweep give the
    same bytes before and after filtered calls on the same workspace."""
    main, nbs = _front_end_inputs(scene_inputs)
    rng = nbs[0]["range_main"]

    def reference():
        return hip.sgm_depth_for_view(main, nbs[:2], num_steps=PLANES)

    def consensus():
        return hip.sgm_depth_for_view(main, nbs, num_steps=PLANES, consensus=True,
                                      want_checked=True)

    def sweep():
        return hip.sgm_sweep_for_view(main, nbs, rng, num_steps=PLANES)
    before = (reference(), consensus(), sweep())
    filtered = [hip.sgm_depth_for_view(main, nbs[:2], num_steps=PLANES, **FILTER),
                hip.sgm_depth_for_view(main, nbs, num_steps=PLANES, consensus=True, **FILTER),
                hip.sgm_sweep_for_view(main, nbs, rng, num_steps=PLANES, **FILTER)["depth"],
                hip.sgm_filter_speckles(before[0], 50, 0.95)[0]]
    after = (reference(), consensus(), sweep())
    for a, b in zip(before, after):
        _same(a, b)
    assert not np.array_equal(filtered[0], before[0])
    assert not np.array_equal(filtered[1], before[1]["depth"])
    assert not np.array_equal(filtered[2], before[2]["depth"])
    assert (before[0] != 0).mean() > 0.5
