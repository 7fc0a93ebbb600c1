"""GPU parity of the opt-in multi-view photo-consistency test of the SGM front
end (include/smvs_hip.h, "Multi-view photo-consistency
test"): the kernel alone against the numpy restatement tests/sgm_photo_ref.py on
the sphere scene and on small and odd shapes, the three front ends against the
restatement applied to their own output with the test off, the host layers, and
the test off against the entries it extends.  The definition fixes every
operation: every comparison of a map is array_equal or tobytes."""
import ctypes as C
import os

import numpy as np
import pytest

import sgm_filter_ref as filter_ref      # tests/sgm_filter_ref.py
import sgm_photo_ref as ref              # tests/sgm_photo_ref.py

pytestmark = pytest.mark.gpu

F = np.float32
N_NEIGHBORS = 6
PLANES = 64
PHOTO = dict(photo_radius=2, photo_best_k=2, photo_min_views=2, photo_min_score=0.49)


@pytest.fixture(scope="module")
def hip():
    import smvs_amd
    if smvs_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on a GPU")
    return smvs_amd


@pytest.fixture(scope="module")
def scene_inputs():
    from smvs_amd import synth
    return synth.pipeline_inputs("sphere", 384, 256, N_NEIGHBORS, flen=1.2)


def _front_end_inputs(inputs, n):
    """(main image, the n neighbours) at SGM scale with both reprojections and
    depth ranges (tests/test_gpu_sgm_merge.py)"""
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


@pytest.fixture(scope="module")
def front(scene_inputs):
    """the scene at SGM scale (192 x 128): the main image, the six neighbours"""
    return _front_end_inputs(scene_inputs, N_NEIGHBORS)


@pytest.fixture(scope="module")
def reference_map(hip, front):
    """the view's two-neighbour reference map, from the device (the oracle's, to
    the bit: tests/test_gpu_front.py)"""
    main, nbs = front
    depth = hip.sgm_depth_for_view(main, nbs[:2], num_steps=PLANES)
    depth.setflags(write=False)
    return depth


_SCORES = {}


def _scores(front, depth, radius):
    """the restatement's scores of all six witnesses on `depth`: once per radius"""
    if radius not in _SCORES:
        main, nbs = front
        score, defined = ref.scores(main, depth, nbs, radius)
        score.setflags(write=False)
        defined.setflags(write=False)
        _SCORES[radius] = (score, defined)
    return _SCORES[radius]


# ------------------------------------------------- 1. the kernel on the scene
@pytest.mark.parametrize("radius", [1, 2, 3])
def test_kernel_matches_the_restatement_on_the_sphere_scene(hip, front, reference_map, radius):
    """1. smvs_sgm_photo_check == the restatement on the view's reference map, for
    n = 1, 2, 3, 6 witnesses, (best_k, min_views) = (1, 1), (2, 2), (0, 5) and
    min_score = -1, 0.25, 0.49: out, confidence and views.  Where best_k or
    min_views exceeds n -- (2, 2) at n = 1, (0, 5) below n = 5 -- the options are
    outside the accepted set and the entry has to refuse them, which is what is
    asserted for those combinations.

    Counted on the CPU on this map at n = 6, r = 2: the views histogram over
    2 .. 6 is 54 / 1122 / 1359 / 868 / 18538; (2, 2, 0.49) drops 721 pixels;
    2786 defined scores are negative."""
    from smvs_amd import _capi
    main, nbs = front
    depth = reference_map
    score, defined = _scores(front, depth, radius)
    valid = depth > 0
    if radius == 2:
        # the comparison is not empty
        _, conf, views = ref.fold(depth, score, defined, 2, 2, 0.49)
        hist = np.bincount(views[valid], minlength=7)
        dropped = int((valid & (conf < F(0.49))).sum())
        kept = int((valid & ~(conf < F(0.49))).sum())
        few = int((valid & (ref.fold(depth, score, defined, 0, 5, -1.0)[1] == -1.0)).sum())
        negative = int((defined & valid[None] & (score < 0)).sum())
        print("views histogram %s; dropped %d, kept %d; min_views 5: %d at -1; negative "
              "scores %d" % (hist.tolist(), dropped, kept, few, negative))
        assert (hist > 0).sum() >= 4 and dropped >= 300 and kept >= 15000
        assert few >= 1000 and negative >= 1
    for n in (1, 2, 3, 6):
        for best_k, min_views in ((1, 1), (2, 2), (0, 5)):
            for min_score in (-1.0, 0.25, 0.49):
                tag = (radius, n, best_k, min_views, min_score)
                if best_k > n or min_views > n:
                    with pytest.raises(_capi.SmvsError) as e:
                        hip.sgm_photo_check(main, depth, nbs[:n], radius, best_k, min_views,
                                            min_score)
                    assert "n_neighbors + n_witness" in str(e.value), tag
                    continue
                want = ref.fold(depth, score[:n], defined[:n], best_k, min_views, min_score)
                got = hip.sgm_photo_check(main, depth, nbs[:n], radius, best_k, min_views,
                                          min_score)
                assert got[2].dtype == np.uint8 and np.array_equal(got[2], want[2]), tag
                assert got[1].dtype == F and np.array_equal(got[1], want[1]), tag
                assert got[0].tobytes() == want[0].tobytes(), tag


# ---------------------------------------------- 2. small and odd shapes
SHAPES = [(1, 1), (1, 70), (70, 1), (5, 3), (33, 31), (65, 63)]     # (w, h)


def _small_case(w, h):
    """A random main image and depth map (with 0, -1, NaN and inf among the
    depths) and four witnesses: a perturbed similarity onto an image of the main
    image's size, one onto an image of another size (47 x 29 against 65 x 63),
    one wholly out of view, one behind the camera."""
    rng = np.random.default_rng(1000 * w + h)
    main = rng.integers(0, 256, (h, w)).astype(np.uint8)
    depth = rng.uniform(0.5, 2.0, (h, w)).astype(F)
    flat = depth.reshape(-1)
    for k, special in enumerate((0.0, -1.0, np.nan, np.inf)):
        flat[(7 * k + 3) % flat.size::23] = special
    other = (47, 29) if (w, h) == (65, 63) else (w + 3, h + 2)

    def similarity(nw, nh):
        a = rng.uniform(-0.05, 0.05)
        s = 0.9 * min(nw / w, nh / h)
        M = np.array([[s * np.cos(a), -s * np.sin(a), 0.04 * nw],
                      [s * np.sin(a), s * np.cos(a), 0.04 * nh],
                      [0.0, 0.0, 1.0]])
        M += rng.uniform(-1e-3, 1e-3, (3, 3))
        return M.astype(F), rng.uniform(-0.02, 0.02, 3).astype(F)
    wits = []
    for nw, nh in ((w, h), other):
        M, t = similarity(nw, nh)
        wits.append(dict(image=rng.integers(0, 256, (nh, nw)).astype(np.uint8), M_fwd=M, t_fwd=t))
    M, t = similarity(w, h)
    wits.append(dict(wits[0], M_fwd=M, t_fwd=t + np.array([1e4, 0, 0], F)))     # out of view
    wits.append(dict(wits[0], M_fwd=M, t_fwd=t + np.array([0, 0, -100], F)))    # p2 < 0
    return main, depth, wits


@pytest.mark.parametrize("w,h", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_kernel_on_small_and_odd_shapes(hip, w, h):
    """2. The kernel alone where the image is smaller than a tile, smaller than
    the window, one pixel wide, and just across the edges of the 32 x 8 tile;
    witnesses of another size, out of view and behind the camera; depths that are
    not valid; out in place, confidence and views NULL."""
    from smvs_amd import _capi, device
    lib = _capi.load()
    main, depth, wits = _small_case(w, h)
    seen = 0
    for radius in (1, 2, 3):
        for best_k, min_views, min_score in ((0, 1, 0.0), (1, 2, -1.0), (2, 0, 0.1)):
            want = ref.photo_check(main, depth, wits, radius, best_k, min_views, min_score)
            tag = (w, h, radius, best_k, min_views, min_score)
            got = hip.sgm_photo_check(main, depth, wits, radius, best_k, min_views, min_score)
            assert np.array_equal(got[2], want[2]), tag
            assert np.array_equal(got[1], want[1]), tag
            assert got[0].tobytes() == want[0].tobytes(), tag
            assert want[2].max() <= 2
            seen = max(seen, int(want[2].max()))
            # in place, without the two optional outputs
            keep = []
            arr = device._sgm_neighbors(device._sgm_witnesses([], wits), keep)
            opts = device.SgmPhotoOptions(radius, best_k, min_views, min_score)
            buf = depth.copy()
            fp = C.POINTER(C.c_float)
            _capi.check(lib.smvs_sgm_photo_check(
                0, main.ctypes.data_as(C.POINTER(C.c_uint8)), w, h, buf.ctypes.data_as(fp), arr,
                len(wits), C.byref(opts), buf.ctypes.data_as(fp), None, None))
            assert buf.tobytes() == want[0].tobytes(), tag
    if min(w, h) >= 31:
        # (the comparison is not empty: both in-view witnesses are defined somewhere)
        assert seen == 2


# ------------------------------------------------------- 3. the three fronts
def _compose(front, off_depth, n_all, speckle):
    main, nbs = front
    out, conf, views = ref.photo_check(main, off_depth, nbs[:n_all], 2, 2, 2, 0.49)
    if speckle:
        out = filter_ref.filter_speckles(out, 50, 0.95)[0]
    return out, conf, views


@pytest.mark.parametrize("speckle", [False, True], ids=["alone", "speckle"])
@pytest.mark.parametrize("case", ["reference-2+4", "consensus-3+3", "sweep-6+0", "sweep-2+4"])
def test_fronts_with_the_test(hip, front, case, speckle):
    """3. Each front with the test (and with the speckle removal behind it) is the
    restatement applied to the same entry's own output with the test off, then
    sgm_filter_ref.filter_speckles: the order is pinned by this.  confidence and
    views are compared too; checked and support are those of the call without
    the test."""
    main, nbs = front
    n = int(case.split("-")[1][0])
    kw = dict(speckle_size=50, speckle_ratio=0.95) if speckle else {}
    rng = nbs[0]["range_main"]
    if case.startswith("sweep"):
        def run(**more):
            return hip.sgm_sweep_for_view(main, nbs[:n], rng, num_steps=PLANES, **more)
    elif case.startswith("consensus"):
        def run(**more):
            return hip.sgm_depth_for_view(main, nbs[:n], num_steps=PLANES, consensus=True,
                                          want_checked=True, **more)
    else:
        def run(**more):
            got = hip.sgm_depth_for_view(main, nbs[:n], num_steps=PLANES, **more)
            return got if isinstance(got, dict) else dict(depth=got)
    off = run()
    got = run(witnesses=nbs[n:], **PHOTO, **kw)
    want = _compose(front, off["depth"], N_NEIGHBORS, speckle)
    dropped = int(((off["depth"] > 0) & (ref.photo_check(main, off["depth"], nbs, 2, 2, 2,
                                                         0.49)[0] == 0)).sum())
    print("%s: %d of %d valid pixels dropped by the test" % (case, dropped,
                                                            int((off["depth"] > 0).sum())))
    assert dropped >= 10 and (want[0] != 0).mean() > 0.5
    assert np.array_equal(got["views"], want[2])
    assert np.array_equal(got["confidence"], want[1])
    assert got["depth"].tobytes() == want[0].tobytes()
    for key in ("checked", "support", "argmin"):
        assert (key in got) == (key in off)
        if key in off:
            assert np.array_equal(got[key], off[key]), key
    if speckle:
        # the other order is another map
        other = ref.photo_check(main, filter_ref.filter_speckles(off["depth"], 50, 0.95)[0],
                                nbs, 2, 2, 2, 0.49)[0]
        if not np.array_equal(other, want[0]):
            assert not np.array_equal(got["depth"], other)


def test_raw_images_with_the_test(hip, front, scene_inputs):
    """3. (cont.) Raw three-channel images, desaturated and halved on the device
    once per view: the reference front at 2 + 4 and the sweep at 2 + 4 give the
    maps of the SGM-scale calls."""
    main, nbs = front
    raw = [dict(nb, image=scene_inputs["images"][k + 1]) for k, nb in enumerate(nbs)]
    rng = nbs[0]["range_main"]
    a = hip.sgm_depth_for_view(main, nbs[:2], num_steps=PLANES, witnesses=nbs[2:], **PHOTO)
    b = hip.sgm_depth_for_view(scene_inputs["images"][0], raw[:2], num_steps=PLANES, halvings=1,
                               witnesses=raw[2:], **PHOTO)
    for key in ("depth", "confidence", "views"):
        assert a[key].tobytes() == b[key].tobytes(), key
    a = hip.sgm_sweep_for_view(main, nbs[:2], rng, num_steps=PLANES, witnesses=nbs[2:], **PHOTO)
    b = hip.sgm_sweep_for_view(scene_inputs["images"][0], raw[:2], rng, num_steps=PLANES,
                               halvings=1, witnesses=raw[2:], **PHOTO)
    for key in ("depth", "confidence", "views", "support"):
        assert a[key].tobytes() == b[key].tobytes(), key
    assert (a["views"] >= 5).mean() > 0.5


# ------------------------------------------------------- 4. the host layers
def test_host_mirror_with_the_test(hip, front, scene_inputs):
    """4. host.sgm_depth with photo_radius = 2 is the restatement on the mirror's
    own map with the test off, for each of the three front ends; all six
    neighbours of the inputs are witnesses, or the first photo_witnesses."""
    from smvs_amd import host
    main, nbs = front
    for kw in (dict(), dict(neighbors=3, consensus=True), dict(neighbors=3, sweep=True)):
        off = host.sgm_depth(scene_inputs, 1, num_steps=PLANES, **kw)
        want = ref.photo_check(main, off, nbs, 2, 2, 2, 0.49)
        got = host.sgm_depth(scene_inputs, 1, num_steps=PLANES, photo_radius=2, **kw)
        assert ((off > 0) & (want[0] == 0)).sum() >= 10 and (want[0] != 0).mean() > 0.5
        assert got[0].tobytes() == want[0].tobytes(), kw
        assert np.array_equal(got[1], want[1]), kw
    # the other options arrive: four witnesses, the best 3 of at least 3, 0.3,
    # the speckle removal behind the test
    off = host.sgm_depth(scene_inputs, 1, num_steps=PLANES)
    want = ref.photo_check(main, off, nbs[:4], 2, 3, 3, 0.3)
    got = host.sgm_depth(scene_inputs, 1, num_steps=PLANES, photo_radius=2, photo_best_k=3,
                         photo_min_views=3, photo_min_score=0.3, photo_witnesses=4,
                         speckle_size=50)
    assert got[0].tobytes() == filter_ref.filter_speckles(want[0], 50, 0.95)[0].tobytes()
    assert np.array_equal(got[1], want[1])
    # fewer witnesses than the front end uses: the front's own
    got = host.sgm_depth(scene_inputs, 1, num_steps=PLANES, photo_radius=1, photo_witnesses=1)
    want = ref.photo_check(main, off, nbs[:2], 1, 2, 2, 0.49)
    assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1])


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


def test_reconstruct_scene_with_the_test(hip, tmp_path):
    """4. (cont.) ReconSettings::sgm_photo_radius on a small written scene: the
    smvs-sgm embedding of the run is the restatement on the map of the
    reference's merge over the two neighbours ViewSelection chose first, with the
    view's three neighbours as witnesses; smvs-sgm-confidence is its confidence.
    A scene that has smvs-sgm embeddings already needs force_sgm."""
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
    main, nbs = _front_end_inputs(sel, 3)
    off = hip.sgm_depth_for_view(main, nbs[:2], num_steps=PLANES)
    want = ref.photo_check(main, off, nbs, 2, 2, 2, 0.49)
    assert ((off > 0) & (want[0] == 0)).sum() >= 10 and (want[0] != 0).mean() > 0.3
    path = str(tmp_path / "scene")
    os.makedirs(path)
    mve_scene.write_scene(path, inputs)
    run = dict(view_ids=[0], num_neighbors=3, min_neighbors=2, output_scale=2,
               sgm_num_steps=PLANES)
    done, skipped, _ = host.reconstruct_scene(path, **run)
    assert done == [0] and skipped == 0
    view = os.path.join(path, "views", "view_0000.mve")
    assert np.array_equal(mve_scene.load_mvei(os.path.join(view, "smvs-sgm.mvei")),
                          _stored(sel, off))
    assert not os.path.exists(os.path.join(view, "smvs-sgm-confidence.mvei"))
    done, skipped, _ = host.reconstruct_scene(path, sgm_photo_radius=2, force_sgm=True,
                                              force_recon=True, **run)
    assert done == [0] and skipped == 0
    got = mve_scene.load_mvei(os.path.join(view, "smvs-sgm.mvei"))
    assert got.shape == (128, 192)
    assert np.array_equal(got, _stored(sel, want[0]))
    conf = mve_scene.load_mvei(os.path.join(view, "smvs-sgm-confidence.mvei"))
    assert conf.dtype == F and np.array_equal(conf, want[1])


# ------------------------------------------------------------ 5. off is off
K_NAMES = ["census", "warp", "cost", "paths", "wta", "lr_check", "merge", "bilateral"]


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
            assert a[key].tobytes() == b[key].tobytes(), key
    else:
        assert a.tobytes() == b.tobytes()


def test_radius_zero_is_the_filtered_entry(hip, front, scene_inputs):
    """5. The two new entries with radius 0 give the bytes and the launches of the
    `_filtered` entries, whatever the other three options; with the test on they
    add one launch of class merge."""
    from smvs_amd import _capi, device
    lib = _capi.load()
    main, nbs = front
    raw = [dict(nb, image=scene_inputs["images"][k + 1]) for k, nb in enumerate(nbs)]
    rng = nbs[0]["range_main"]
    filt = dict(uniqueness=10, uniqueness_window=4, speckle_size=50, speckle_ratio=0.95)

    def entries(**kw):
        return [
            lambda: hip.sgm_depth_for_view(main, nbs[:2], num_steps=PLANES, **filt, **kw),
            lambda: hip.sgm_depth_for_view(main, nbs[:3], num_steps=PLANES, consensus=True,
                                           want_checked=True, **filt, **kw),
            lambda: hip.sgm_depth_for_view(scene_inputs["images"][0], raw[:2], num_steps=PLANES,
                                           halvings=1, **kw),
            lambda: hip.sgm_sweep_for_view(main, nbs[:3], rng, num_steps=PLANES,
                                           want_volumes=True, **filt, **kw),
            lambda: hip.sgm_sweep_for_view(scene_inputs["images"][0], raw[:3], rng,
                                           num_steps=PLANES, halvings=1, **kw)]
    parents = [_launches(lib, fn) for fn in entries()]
    for off in ((0, 0, 0, -1.0), (0, 2, 1, 1.0), (0, 2, 2, 0.5)):
        kw = dict(zip(("photo_radius", "photo_best_k", "photo_min_views", "photo_min_score"), off))
        assert device._sgm_photo(*off, None) is not None
        for k, fn in enumerate(entries(**kw)):
            out, cnt = _launches(lib, fn)
            if isinstance(out, dict):
                assert out.pop("confidence") is None and out.pop("views") is None
                if not isinstance(parents[k][0], dict):
                    out = out["depth"]
            _same(out, parents[k][0])
            assert cnt == parents[k][1], (k, kw)
    for k in (0, 1, 3):
        _, cnt = _launches(lib, entries(**PHOTO)[k])
        want = dict(parents[k][1])
        want["merge"] += 1
        assert cnt == want, k


def test_existing_entries_keep_their_bytes_around_a_call_with_the_test(hip, front):
    """5. (cont.) The reference front end, the consensus and the sweep give the
    same bytes before and after calls with the test on the same workspace."""
    main, nbs = front
    rng = nbs[0]["range_main"]

    def reference():
        return hip.sgm_depth_for_view(main, nbs[:2], num_steps=PLANES)

    def consensus():
        return hip.sgm_depth_for_view(main, nbs[:3], num_steps=PLANES, consensus=True,
                                      want_checked=True)

    def sweep():
        return hip.sgm_sweep_for_view(main, nbs, rng, num_steps=PLANES)
    before = (reference(), consensus(), sweep())
    tested = [hip.sgm_depth_for_view(main, nbs[:2], num_steps=PLANES, witnesses=nbs[2:],
                                     **PHOTO)["depth"],
              hip.sgm_depth_for_view(main, nbs[:3], num_steps=PLANES, consensus=True,
                                     witnesses=nbs[3:], **PHOTO)["depth"],
              hip.sgm_sweep_for_view(main, nbs, rng, num_steps=PLANES, **PHOTO)["depth"],
              hip.sgm_photo_check(main, before[0], nbs)[0]]
    after = (reference(), consensus(), sweep())
    for a, b in zip(before, after):
        _same(a, b)
    assert not np.array_equal(tested[0], before[0])
    assert not np.array_equal(tested[1], before[1]["depth"])
    assert not np.array_equal(tested[2], before[2]["depth"])
    assert tested[3].tobytes() == tested[0].tobytes()
    assert (before[0] != 0).mean() > 0.5
