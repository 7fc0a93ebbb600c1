"""GPU parity of the opt-in multi-view plane refinement sweeps of the SGM front
end (include/smvs_hip.h, "Multi-view plane refinement
sweeps"): the kernels alone against the numpy restatement tests/sgm_refine_ref.py
on the sphere scene and on small and odd shapes, the sweeps off against the photo
test's entries, the three front ends against the restatement applied to their own
output with the photo test off, the host layers, and determinism.  The definition
fixes every operation: every comparison of a map is array_equal or tobytes."""
import ctypes as C
import os

import numpy as np
import pytest

import sgm_filter_ref as filter_ref      # tests/sgm_filter_ref.py
import sgm_refine_ref as ref             # tests/sgm_refine_ref.py

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
    return synth.pipeline_inputs("sphere", 192, 128, N_NEIGHBORS, flen=1.2)


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
    """the scene at SGM scale (96 x 64): the main image, the six neighbours"""
    main, nbs = _front_end_inputs(scene_inputs, N_NEIGHBORS)
    assert main.shape == (64, 96)
    return main, nbs


@pytest.fixture(scope="module")
def reference_map(hip, front):
    """the view's two-neighbour reference map, from the device"""
    main, nbs = front
    depth = hip.sgm_depth_for_view(main, nbs[:2], num_steps=PLANES)
    depth.setflags(write=False)
    return depth


def _same4(got, want, tag):
    """(out, slant, confidence, views) of the device against the restatement's"""
    assert got[3].dtype == np.uint8 and np.array_equal(got[3], want[3]), tag
    assert got[2].dtype == F and got[2].tobytes() == want[2].tobytes(), tag
    assert got[1].dtype == F and got[1].shape == want[1].shape, tag
    assert got[1].tobytes() == want[1].tobytes(), tag
    assert got[0].dtype == F and got[0].tobytes() == want[0].tobytes(), tag


# ------------------------------------------------- 1. the kernels on the scene
ROWS = [(1, 1, 1, 1), (2, 2, 2, 2), (2, 6, 2, 2), (3, 3, 0, 2)]    # r, n, best_k, min_views
SWEEPS = [(1, 0), (2, 2), (3, 1)]                                  # sweeps, samples
GRID = [(row, ss, fill, 1) for row in ROWS for ss in SWEEPS for fill in (0, 1)] \
    + [((2, 6, 2, 2), (2, 2), fill, 12345) for fill in (0, 1)]


@pytest.mark.parametrize("row,ss,fill,seed", GRID,
                         ids=["r%d-n%d-%dof%d-s%dx%d-fill%d-seed%d" % (g[0] + g[1] + g[2:])
                              for g in GRID])
def test_kernels_match_the_restatement_on_the_sphere_scene(hip, front, reference_map, row, ss,
                                                          fill, seed):
    """1. smvs_sgm_plane_refine == the restatement on the view's reference map, on
    all four outputs, for (r, n, best_k of min_views) = (1, 1, 1 of 1), (2, 2, 2 of
    2), (2, 6, 2 of 2), (3, 3, all of 2), each at (sweeps, samples) = (1, 0),
    (2, 2), (3, 1), fill 0 and 1, min_score 0.49; a second seed at (2, 6, 2 of 2).
    The comparison is not empty: at least 5 % of the valid pixels change their
    depth, and with fill = 1 at least one hole is filled (with fill = 0 none can
    be).

    Counted on the CPU on this map (5320 valid pixels, 824 holes), before the end
    rule drops anything: at (1, 0) 1992 .. 2093 valid pixels change depth, at
    (2, 2) 4586 .. 4939, at (3, 1) 4876 .. 4961; with fill = 1 254 .. 452 holes
    are filled at (1, 0), 371 .. 723 at (2, 2), 431 .. 820 at (3, 1), the most at
    n = 6.  At (2, 6, 2 of 2), (2, 2), fill 1: 9227 adoptions by propagation and
    4265 by perturbation with seed 1, 9207 and 4201 with seed 12345."""
    main, nbs = front
    depth = reference_map
    radius, n, best_k, min_views = row
    sweeps, samples = ss
    kw = dict(radius=radius, best_k=best_k, min_views=min_views, min_score=0.49, sweeps=sweeps,
              samples=samples, seed=seed, fill=fill)
    counts = {}
    want = ref.plane_refine(main, depth, nbs[:n], counts=counts, **kw)
    # (the depth before the end rule drops it: min_score -1 of the same run)
    loose = ref.plane_refine(main, depth, nbs[:n], **dict(kw, min_score=-1.0))[0]
    valid = depth > 0
    changed = int((valid & (loose != depth)).sum())
    filled = int((~valid & (loose > 0)).sum())
    print("%s: %d of %d valid pixels changed depth, %d of %d holes filled, adoptions %s"
          % (kw, changed, valid.sum(), filled, (~valid).sum(), counts))
    assert changed >= 0.05 * valid.sum()
    assert (filled >= 1) if fill else (filled == 0)
    got = hip.sgm_plane_refine(main, depth, nbs[:n], **kw)
    _same4(got, want, kw)


# ---------------------------------------------- 2. small and odd shapes
SHAPES = [(1, 1), (1, 70), (70, 1), (5, 3), (33, 31), (65, 63)]     # (w, h)


def _small_case(w, h):
    """A random main image and depth map (with 0, -1, NaN and inf among the
    depths) and four witnesses: a perturbed similarity onto an image of the main
    image's size, one onto an image of another size (47 x 29 against 65 x 63),
    one wholly out of view, one behind the camera (the case of
    tests/test_gpu_sgm_photo.py, rebuilt)."""
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


@pytest.mark.parametrize("fill", [0, 1])
@pytest.mark.parametrize("w,h", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_kernels_on_small_and_odd_shapes(hip, w, h, fill):
    """2. The kernels alone where the image is smaller than a tile, smaller than
    the window, one pixel wide or high, and just across the edges of the 32 x 8
    and 64 x 8 tiles (odd widths: the colour mapping at the right edge); witnesses
    of another size, out of view and behind the camera; depths that are not
    valid.  2 sweeps, 2 samples, r = 1, 2, 3; out in place, the optional outputs
    NULL."""
    from smvs_amd import _capi, device
    lib = _capi.load()
    main, depth, wits = _small_case(w, h)
    moved = 0
    for radius, best_k, min_views, min_score in ((1, 0, 1, 0.0), (2, 1, 2, -1.0), (3, 2, 0, 0.1)):
        kw = dict(radius=radius, best_k=best_k, min_views=min_views, min_score=min_score,
                  sweeps=2, samples=2, depth_step=0.05, slant_step=0.02, seed=7, fill=fill)
        counts = {}
        want = ref.plane_refine(main, depth, wits, counts=counts, **kw)
        got = hip.sgm_plane_refine(main, depth, wits, **kw)
        _same4(got, want, (w, h, kw))
        moved += counts["propagation"] + counts["perturbation"]
        # in place, without the three optional outputs
        keep = []
        arr = device._sgm_neighbors(device._sgm_witnesses([], wits), keep)
        photo = device.SgmPhotoOptions(radius, best_k, min_views, min_score)
        refine = device.SgmRefineOptions(2, 2, 0.05, 0.02, 7, fill)
        buf = depth.copy()
        fp = C.POINTER(C.c_float)
        _capi.check(lib.smvs_sgm_plane_refine(
            0, main.ctypes.data_as(C.POINTER(C.c_uint8)), w, h, buf.ctypes.data_as(fp), arr,
            len(wits), C.byref(photo), C.byref(refine), buf.ctypes.data_as(fp), None, None, None))
        assert buf.tobytes() == want[0].tobytes(), (w, h, kw)
    print("%d x %d, fill %d: %d adoptions" % (w, h, fill, moved))
    if min(w, h) >= 31:
        # (the comparison is not empty)
        assert moved >= 100


# --------------------------------------------------------- 3. off is off
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
    assert sorted(a) == sorted(b)
    for key in a:
        if a[key] is None:
            assert b[key] is None, key
        else:
            assert a[key].tobytes() == b[key].tobytes(), key


def test_no_sweeps_is_the_photo_test(hip, front, reference_map, scene_inputs):
    """3. With sweeps = 0 smvs_sgm_plane_refine gives smvs_sgm_photo_check's three
    outputs and zero slants; the two `_refine` view entries give the bytes and the
    launches of the `_photo` entries for all three front ends, whatever the other
    five options; with the sweeps on they make 1 + 2 sweeps + 1 launches of class
    merge where the photo test makes one."""
    from smvs_amd import _capi, device
    lib = _capi.load()
    main, nbs = front
    for radius, n, best_k, min_views in ROWS:
        want = hip.sgm_photo_check(main, reference_map, nbs[:n], radius, best_k, min_views, 0.49)
        got = hip.sgm_plane_refine(main, reference_map, nbs[:n], radius, best_k, min_views, 0.49,
                                   sweeps=0, samples=5, fill=0)
        assert got[0].tobytes() == want[0].tobytes()
        assert got[2].tobytes() == want[1].tobytes() and np.array_equal(got[3], want[2])
        assert got[1].shape == (64, 96, 2) and not got[1].any()
    raw = [dict(nb, image=scene_inputs["images"][k + 1]) for k, nb in enumerate(nbs)]
    rng = nbs[0]["range_main"]
    filt = dict(uniqueness=10, uniqueness_window=4, speckle_size=50, speckle_ratio=0.95)

    def entries(**kw):
        return [
            lambda: hip.sgm_depth_for_view(main, nbs[:2], num_steps=PLANES, witnesses=nbs[2:],
                                           **PHOTO, **filt, **kw),
            lambda: hip.sgm_depth_for_view(main, nbs[:3], num_steps=PLANES, consensus=True,
                                           want_checked=True, witnesses=nbs[3:], **PHOTO, **filt,
                                           **kw),
            lambda: hip.sgm_sweep_for_view(main, nbs[:3], rng, num_steps=PLANES,
                                           want_volumes=True, witnesses=nbs[3:], **PHOTO, **filt,
                                           **kw),
            lambda: hip.sgm_sweep_for_view(scene_inputs["images"][0], raw[:3], rng,
                                           num_steps=PLANES, halvings=1, **PHOTO, **kw)]
    parents = [_launches(lib, fn) for fn in entries()]
    for off in (dict(refine_samples=0), dict(refine_samples=8, refine_depth_step=1.0,
                                             refine_slant_step=0.0, refine_seed=9, refine_fill=0)):
        assert device._sgm_refine(0, *[off.get("refine_" + k, d) for k, d in
                                       zip(("samples", "depth_step", "slant_step", "seed", "fill"),
                                           device.SGM_REFINE_DEFAULTS[1:])]) is not None
        for k, fn in enumerate(entries(**off)):
            out, cnt = _launches(lib, fn)
            assert out.pop("slant") is None
            _same(out, parents[k][0])
            assert cnt == parents[k][1], (k, off)
    for k in (0, 1, 2):
        out, cnt = _launches(lib, entries(refine_sweeps=2)[k])
        want = dict(parents[k][1])
        want["merge"] += 2 * 2 + 1
        assert cnt == want, k
        assert out["slant"].shape == (64, 96, 2) and out["slant"].any()
    # and the photo test off, with the sweeps' other options changed: the
    # `_filtered` entries' bytes
    plain = hip.sgm_depth_for_view(main, nbs[:2], num_steps=PLANES, **filt)
    got = hip.sgm_depth_for_view(main, nbs[:2], num_steps=PLANES, refine_seed=3, **filt)
    assert got["depth"].tobytes() == plain.tobytes()
    assert got["confidence"] is None and got["slant"] is None


# ------------------------------------------------------- 4. the three fronts
_COMPOSE = dict(sweeps=2, samples=2, depth_step=0.02, slant_step=0.01, seed=1, fill=1)


@pytest.mark.parametrize("case", ["reference-2+4", "consensus-3+3", "sweep-6+0"])
def test_fronts_with_the_sweeps_then_the_speckle_removal(hip, front, case):
    """4. Each front with the sweeps and the speckle removal behind them is the
    restatement applied to the same entry's own output with the photo test off,
    then sgm_filter_ref.filter_speckles: the order is pinned by this.  slant,
    confidence and views are compared too; checked and support are those of the
    call without the sweeps."""
    main, nbs = front
    n = int(case.split("-")[1][0])
    kw = dict(speckle_size=50, speckle_ratio=0.95)
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
    got = run(witnesses=nbs[n:], refine_sweeps=2, **PHOTO, **kw)
    out, slant, conf, views = ref.plane_refine(main, off["depth"], nbs, 2, 2, 2, 0.49, **_COMPOSE)
    want = filter_ref.filter_speckles(out, 50, 0.95)[0]
    changed = int(((off["depth"] > 0) & (out != off["depth"])).sum())
    print("%s: %d of %d valid pixels changed or dropped, %d holes filled"
          % (case, changed, int((off["depth"] > 0).sum()),
             int((~(off["depth"] > 0) & (out > 0)).sum())))
    assert changed >= 100 and (want != 0).mean() > 0.5
    assert np.array_equal(got["views"], views)
    assert got["confidence"].tobytes() == conf.tobytes()
    assert got["slant"].tobytes() == slant.tobytes()
    assert got["depth"].tobytes() == want.tobytes()
    for key in ("checked", "support", "argmin"):
        assert (key in got) == (key in off)
        if key in off:
            assert np.array_equal(got[key], off[key]), key
    # the other order is another map
    other = ref.plane_refine(main, filter_ref.filter_speckles(off["depth"], 50, 0.95)[0], nbs,
                             2, 2, 2, 0.49, **_COMPOSE)[0]
    if not np.array_equal(other, want):
        assert not np.array_equal(got["depth"], other)


# ------------------------------------------------------- 5. the host layers
def test_host_mirror_with_the_sweeps(hip, front, scene_inputs):
    """5. host.sgm_depth with photo_radius = 2 and refine_sweeps = 2 is the device
    front with the same options -- depth, confidence and slant -- for each of the
    three front ends, all six neighbours of the inputs being witnesses; the other
    options arrive."""
    from smvs_amd import host
    main, nbs = front
    rng = nbs[0]["range_main"]
    for kw, dev in ((dict(), lambda **m: hip.sgm_depth_for_view(main, nbs[:2], **m)),
                    (dict(neighbors=3, consensus=True),
                     lambda **m: hip.sgm_depth_for_view(main, nbs[:3], consensus=True, **m)),
                    (dict(neighbors=3, sweep=True),
                     lambda **m: hip.sgm_sweep_for_view(main, nbs[:3], rng, **m))):
        n = kw.get("neighbors", 2)
        want = dev(num_steps=PLANES, witnesses=nbs[n:], refine_sweeps=2, **PHOTO)
        got = host.sgm_depth(scene_inputs, 1, num_steps=PLANES, photo_radius=2, refine_sweeps=2,
                             **kw)
        assert len(got) == 3 and got[2].shape == (64, 96, 2) and got[2].any()
        assert got[0].tobytes() == want["depth"].tobytes(), kw
        assert got[1].tobytes() == want["confidence"].tobytes(), kw
        assert got[2].tobytes() == want["slant"].tobytes(), kw
    other = dict(refine_sweeps=1, refine_samples=3, refine_depth_step=0.05,
                 refine_slant_step=0.02, refine_seed=77, refine_fill=0)
    want = hip.sgm_depth_for_view(main, nbs[:2], num_steps=PLANES, witnesses=nbs[2:],
                                  speckle_size=50, **PHOTO, **other)
    got = host.sgm_depth(scene_inputs, 1, num_steps=PLANES, photo_radius=2, speckle_size=50,
                         **other)
    assert got[0].tobytes() == want["depth"].tobytes()
    assert got[2].tobytes() == want["slant"].tobytes()
    plain = hip.sgm_depth_for_view(main, nbs[:2], num_steps=PLANES)
    assert not (got[0][~(plain > 0)] > 0).any()      # fill = 0


def _spread_ring_inputs(n=3):
    """The sphere scene of synth.pipeline_inputs at 384 x 256 with the neighbours
    on rings of different radii: ViewSelection keeps one view per distance from
    the main view (tests/test_gpu_sgm_merge.py)."""
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


def _stored(inputs, z):
    """What write_depth_to_view stores for the z-depth map z as "smvs-sgm"
    (tests/test_gpu_sgm_sweep.py)."""
    from smvs_amd import host
    host.optimize(inputs, regularization=0.01, num_iterations=1, min_scale=2, sgm_depth=z)
    return host.last_embeddings()["smvs-sgm"]


def test_reconstruct_scene_with_the_sweeps(hip, tmp_path):
    """5. (cont.) ReconSettings::sgm_refine_sweeps on a small written scene: the
    smvs-sgm, smvs-sgm-confidence and smvs-sgm-slant embeddings of the run are the
    device front's outputs on the two neighbours ViewSelection chose first, with
    the view's three neighbours as witnesses.  A scene that has smvs-sgm
    embeddings already needs force_sgm."""
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
    want = hip.sgm_depth_for_view(main, nbs[:2], num_steps=PLANES, witnesses=nbs[2:],
                                  refine_sweeps=2, **PHOTO)
    photo = hip.sgm_depth_for_view(main, nbs[:2], num_steps=PLANES, witnesses=nbs[2:], **PHOTO)
    assert not np.array_equal(want["depth"], photo["depth"]) and want["slant"].any()
    path = str(tmp_path / "scene")
    os.makedirs(path)
    mve_scene.write_scene(path, inputs)
    run = dict(view_ids=[0], num_neighbors=3, min_neighbors=2, output_scale=2,
               sgm_num_steps=PLANES)
    done, skipped, _ = host.reconstruct_scene(path, sgm_photo_radius=2, **run)
    assert done == [0] and skipped == 0
    view = os.path.join(path, "views", "view_0000.mve")
    assert np.array_equal(mve_scene.load_mvei(os.path.join(view, "smvs-sgm.mvei")),
                          _stored(sel, photo["depth"]))
    assert not os.path.exists(os.path.join(view, "smvs-sgm-slant.mvei"))
    done, skipped, _ = host.reconstruct_scene(path, sgm_photo_radius=2, sgm_refine_sweeps=2,
                                              force_sgm=True, force_recon=True, **run)
    assert done == [0] and skipped == 0
    got = mve_scene.load_mvei(os.path.join(view, "smvs-sgm.mvei"))
    assert got.shape == (128, 192)
    assert np.array_equal(got, _stored(sel, want["depth"]))
    conf = mve_scene.load_mvei(os.path.join(view, "smvs-sgm-confidence.mvei"))
    assert conf.dtype == F and conf.tobytes() == want["confidence"].tobytes()
    slant = mve_scene.load_mvei(os.path.join(view, "smvs-sgm-slant.mvei"))
    assert slant.dtype == F and slant.shape == (128, 192, 2)
    assert slant.tobytes() == want["slant"].tobytes()


# ------------------------------------------------------------ 6. determinism
def test_the_same_call_twice_gives_the_same_bytes(hip, front, reference_map):
    """6. The half-sweeps work in place; the result does not depend on the order
    in which the blocks run."""
    main, nbs = front
    kw = dict(radius=2, best_k=2, min_views=2, min_score=0.3, sweeps=3, samples=2, seed=5)
    a = hip.sgm_plane_refine(main, reference_map, nbs, **kw)
    b = hip.sgm_plane_refine(main, reference_map, nbs, **kw)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    assert a[1].any()
