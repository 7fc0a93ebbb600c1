"""CPU checks of the opt-in multi-view photo-consistency test of the SGM front
end (include/smvs_hip.h, "Multi-view photo-consistency
test"): the numpy restatement tests/sgm_photo_ref.py pinned against the oracle's
warp and on windows worked out by hand, the edges of the definition, the
argument checks of the three new entries, which need no GPU, and the defaults of
the host mirror and the Python fronts."""
import ctypes as C
import inspect

import numpy as np
import pytest

import sgm_photo_ref as ref              # tests/sgm_photo_ref.py
import sgm_subplane_ref as subplane_ref  # tests/sgm_subplane_ref.py

F = np.float32
INVALID = -1
IDENTITY = dict(M_fwd=np.eye(3, dtype=F), t_fwd=np.zeros(3, F))


# ------------------------------------------------------------------ the sample
def test_sample_is_the_oracles_warp(oracle):
    """On the pair of tests/sgm_subplane_ref.py, for every plane of an 8-plane
    table: every pixel the restatement calls inside has the byte of orc_sgm_warp,
    every pixel it calls outside has byte 0 in the oracle's volume."""
    main, nbr, M, t = subplane_ref.scene_pair()
    h, w = main.shape
    nh, nw = nbr.shape
    D = 8
    depths = oracle.sgm_depths(3, 12, D)
    M32, t32 = np.ascontiguousarray(M, F).reshape(9), np.ascontiguousarray(t, F).reshape(3)
    nbr = np.ascontiguousarray(nbr, np.uint8)
    warped = np.zeros((h, w, D), np.uint8)
    u8p, fp = C.POINTER(C.c_uint8), C.POINTER(C.c_float)
    oracle.lib().orc_sgm_warp(nbr.ctypes.data_as(u8p), C.c_int(nw), C.c_int(nh),
                              M32.ctypes.data_as(fp), t32.ctypes.data_as(fp),
                              depths.ctypes.data_as(fp), C.c_int(D), C.c_int(w), C.c_int(h),
                              warped.ctypes.data_as(u8p))
    yy, xx = np.mgrid[0:h, 0:w]
    n_inside = 0
    for d in range(D):
        B, inside = ref.sample(nbr, M, t, xx, yy, np.full((h, w), depths[d], F))
        assert np.array_equal(B[inside], warped[:, :, d][inside]), d
        assert not warped[:, :, d][~inside].any(), d
        assert not B[~inside].any()
        n_inside += int(inside.sum())
    print("inside: %d of %d samples" % (n_inside, h * w * D))
    assert 0 < n_inside < h * w * D and warped.any()


def _textured(h, w, seed=3):
    return np.random.default_rng(seed).integers(0, 256, (h, w)).astype(np.uint8)


def _score_one(main, wit, radius, depth=1.0, **reprojection):
    nb = dict(IDENTITY, image=wit)
    nb.update(reprojection)
    score, defined = ref.scores(main, np.full(main.shape, depth, F), [nb], radius)
    return score[0], defined[0]


# --------------------------------------------------------------------- by hand
@pytest.mark.parametrize("radius", [1, 2, 3])
def test_scores_by_hand(radius):
    """Under the identity reprojection a pixel's sample is the witness's own
    pixel (p = (x + 0.5, y + 0.5) - 0.5, weights 1, 0, 0, 0)."""
    img = _textured(12, 14)
    h, w = img.shape
    # the witness is the main image: 1.0 wherever the window has contrast; every
    # window is inside (the window's coordinates are clamped to the image)
    score, defined = _score_one(img, img, radius)
    assert defined.all() and (score == 1.0).all()
    # inverted: -1.0 exactly (cov = -va, vb = va)
    score, defined = _score_one(img, 255 - img, radius)
    assert defined.all() and (score == -1.0).all()
    # a flat window is no evidence -- 0.0 -- and still counts as defined
    flat = img.copy()
    flat[:2 * radius + 1, :2 * radius + 1] = 77
    score, defined = _score_one(flat, img, radius)
    assert defined.all() and score[radius, radius] == 0.0 and score[-1, -1] != 0.0
    score, defined = _score_one(img, np.full_like(img, 9), radius)
    assert defined.all() and (score == 0.0).all()
    out, conf, views = ref.fold(np.ones((h, w), F), score[None], defined[None], 0, 1, 0.0)
    assert (views == 1).all() and (conf == 0.0).all() and (out == 1.0).all()
    # half the correlation: the witness agrees on the sign of every step but not
    # on its size -- the score lies strictly between 0 and 1
    score, _ = _score_one(img, (img // 2 + (img % 7)).astype(np.uint8), radius)
    assert ((score > 0) & (score < 1)).all()


@pytest.mark.parametrize("radius", [1, 2, 3])
def test_a_window_that_leaves_the_witness_by_one_sample_is_not_defined(radius):
    """A shift by one pixel (M = I, t = (1, 0, 0), depth 1): the sample of main
    pixel x lies at x + 1 in the witness.  A witness as wide as the
    main image is left by the windows whose last column is the image's last; one
    column more and every window is inside."""
    img = _textured(10, 16)
    h, w = img.shape
    shift = dict(t_fwd=np.array([1, 0, 0], F))
    wide = np.concatenate([img[:, :1], img], axis=1)      # wide[:, x + 1] = img[:, x]
    score, defined = _score_one(img, wide, radius, **shift)
    assert defined.all() and (score == 1.0).all()
    score, defined = _score_one(img, wide[:, :w], radius, **shift)
    # x + radius + 1 <= w - 1, and the clamped windows at the right edge sample
    # column w - 1 of the main image: x = w - 1 - radius is the first to leave
    assert defined[:, :w - 1 - radius].all() and not defined[:, w - 1 - radius:].any()
    assert (score[:, :w - 1 - radius] == 1.0).all()
    # behind the camera (p2 < 0) and a projective depth of 0 (0 / 0): outside
    _, defined = _score_one(img, img, radius, t_fwd=np.array([0, 0, -2], F))
    assert not defined.any()
    _, defined = _score_one(img, img, radius, t_fwd=np.array([0, 0, -1], F))
    assert not defined.any()


def test_sums_of_the_largest_window_stay_below_2_31():
    """7 x 7 samples of 255 on both sides: every sum and every product of the
    definition fits 32 bits; a half-and-half window has the largest variance."""
    N = 49
    SA = SB = N * 255
    SAB = SAA = SBB = N * 255 * 255
    for v in (SA, SAB, N * SAB, SA * SB, N * SAA, SA * SA):
        assert 0 <= v < 2 ** 31
    white = np.full((9, 9), 255, np.uint8)
    sums = ref.window_sums(white, np.ones((9, 9), F), white, IDENTITY["M_fwd"],
                           IDENTITY["t_fwd"], 3)
    assert [int(s[4, 4]) for s in sums[:5]] == [SA, SB, SAB, SAA, SBB] and sums[5].all()
    half = np.zeros((9, 9), np.uint8)
    half[:, :5] = 255
    SA, SB, SAB, SAA, SBB, defined = (s[4, 4] for s in ref.window_sums(
        half, np.ones((9, 9), F), half, IDENTITY["M_fwd"], IDENTITY["t_fwd"], 3))
    va = N * SAA - SA * SA
    assert 0 < va < 2 ** 31 and va * va < 2 ** 53


# ------------------------------------------------------------ the pixel's part
def _scene():
    """A main image and three witnesses that agree with it to different degrees
    (identity reprojection), depth 1 everywhere."""
    img = _textured(16, 20, seed=5)
    noise = np.random.default_rng(6).integers(-60, 60, img.shape)
    wits = [dict(IDENTITY, image=img),
            dict(IDENTITY, image=np.clip(img.astype(int) + noise, 0, 255).astype(np.uint8)),
            dict(IDENTITY, image=_textured(16, 20, seed=7))]
    return img, np.ones(img.shape, F), wits


def test_mean_of_the_best_in_descending_order():
    img, depth, wits = _scene()
    score, defined = ref.scores(img, depth, wits, 2)
    assert defined.all() and (score[0] == 1.0).all()
    assert (score[1] < 1.0).all() and (score[1] > score[2]).all()
    for best_k, want in ((1, score[0]), (2, (score[0] + score[1]) / 2.0),
                         (0, ((score[0] + score[1]) + score[2]) / 3.0),
                         (3, ((score[0] + score[1]) + score[2]) / 3.0)):
        out, conf, views = ref.fold(depth, score, defined, best_k, 1, -1.0)
        assert conf.dtype == F and np.array_equal(conf, want.astype(F)), best_k
        assert (views == 3).all() and out.tobytes() == depth.tobytes()
    # the order of the witnesses does not matter
    again = ref.photo_check(img, depth, wits[::-1], 2, 2, 1, -1.0)[1]
    assert np.array_equal(again, ((score[0] + score[1]) / 2.0).astype(F))
    # best_k above the defined ones: the mean of those there are
    undefined = defined.copy()
    undefined[0] = False
    conf = ref.fold(depth, score, undefined, 3, 1, -1.0)[1]
    assert np.array_equal(conf, ((score[1] + score[2]) / 2.0).astype(F))


def test_a_pixel_exactly_at_the_bound_is_kept():
    img, depth, wits = _scene()
    conf = ref.photo_check(img, depth, wits, 2, 0, 1, -1.0)[1]
    y, x = 7, 9
    own = conf[y, x]
    assert -1.0 < own < 1.0
    out = ref.photo_check(img, depth, wits, 2, 0, 1, float(own))[0]
    assert out[y, x] == depth[y, x]
    out = ref.photo_check(img, depth, wits, 2, 0, 1, float(np.nextafter(own, F(2))))[0]
    assert out[y, x] == 0.0
    # the comparison is the float's: a bound between the two floats rounds to one
    between = (float(own) + float(np.nextafter(own, F(2)))) / 2.0
    assert ref.photo_check(img, depth, wits, 2, 0, 1, between)[0][y, x] == (
        depth[y, x] if F(between) == own else 0.0)


def test_too_few_views_is_minus_one_and_dropped_unless_min_score_is_minus_one():
    img, depth, wits = _scene()
    out, conf, views = ref.photo_check(img, depth, wits, 2, 2, 4, 0.49)
    assert (views == 3).all() and (conf == -1.0).all() and not out.any()
    out, conf, views = ref.photo_check(img, depth, wits, 2, 2, 4, -1.0)
    assert (conf == -1.0).all() and out.tobytes() == depth.tobytes()
    # min_views 0 is min_views 1: no defined witness is -1.0, never 0 / 0
    away = [dict(nb, t_fwd=np.array([0, 0, -2], F)) for nb in wits]
    out, conf, views = ref.photo_check(img, depth, away, 2, 2, 0, -1.0)
    assert (views == 0).all() and (conf == -1.0).all() and out.tobytes() == depth.tobytes()
    assert not ref.photo_check(img, depth, away, 2, 2, 0, -0.99)[0].any()


def test_pixels_that_are_not_valid_keep_their_bits():
    """A NaN with a payload, -0.0, a negative and a zero keep their bits and get
    -1.0f / 0 whatever min_score; an infinite depth is valid, has no defined
    witness (inf / inf) and is dropped."""
    img, depth, wits = _scene()
    depth = depth.copy()
    depth[0, :5] = [np.nan, -0.0, -3.5, 0.0, np.inf]
    depth.view(np.uint32)[0, 0] = 0x7FC12345
    for min_score in (-1.0, 0.49, 1.0):
        out, conf, views = ref.photo_check(img, depth, wits, 1, 2, 2, min_score)
        assert out[0, :4].tobytes() == depth[0, :4].tobytes()
        assert out.view(np.uint32)[0, 0] == 0x7FC12345
        assert out.view(np.uint32)[0, 1] == 0x80000000
        assert (conf[0, :5] == -1.0).all() and (views[0, :5] == 0).all()
        assert out[0, 4] == (np.inf if min_score == -1.0 else 0.0)
    assert (views[1:] == 3).all()


# ------------------------------------------------------------------ the entries
def _hip_lib():
    from smvs_amd import _capi
    lib = _capi.load()
    lib.smvs_last_error.restype = C.c_char_p
    return lib


W, H = 24, 16
ENTRIES = ("smvs_sgm_depth_for_view_raw_photo", "smvs_sgm_sweep_for_view_raw_photo",
           "smvs_sgm_photo_check")
GOOD = (2, 2, 2, 0.49)


def _call(lib, entry, photo=GOOD, n_neighbors=2, n_witness=1, confidence=True, views=True,
          null_photo=False, bad_witness=None, witness_channels=3, filt=(0, 1, 0, 0.95)):
    """one of the three entries on a small image with three views behind it"""
    from smvs_amd import device
    u8p, fp = C.POINTER(C.c_uint8), C.POINTER(C.c_float)
    main = np.full((H, W, 3), 90, np.uint8)
    grey = np.full((H, W), 90, np.uint8)
    alone = entry == "smvs_sgm_photo_check"
    nb = dict(image=grey if alone else main, M_fwd=np.eye(3), t_fwd=[-6, 0, 0], M_bwd=np.eye(3),
              t_bwd=[6, 0, 0], range_main=[1, 8], range_neighbor=[1, 8])
    keep = []
    arr = device._sgm_neighbors([nb] * 16, keep)
    if bad_witness == "image":
        arr[n_neighbors].image = None
    if bad_witness == "size":
        arr[n_neighbors].width = 0
    nch = (C.c_int * 16)(*([3] * 16))
    nch[min(n_neighbors, 15)] = witness_channels
    depth = np.ones((H, W), F)
    conf = np.zeros((H, W), F).ctypes.data_as(fp) if confidence else None
    vw = np.zeros((H, W), np.uint8).ctypes.data_as(u8p) if views else None
    p = None if null_photo else C.byref(device.SgmPhotoOptions(*photo))
    f = C.byref(device.SgmFilterOptions(*filt))
    p1, p2 = C.c_uint16(6), C.c_uint16(96)
    mp, dp = main.ctypes.data_as(u8p), depth.ctypes.data_as(fp)
    if alone:
        return lib.smvs_sgm_photo_check(0, grey.ctypes.data_as(u8p), W, H, dp, arr,
                                        n_neighbors + n_witness, p, dp, conf, vw)
    if entry == ENTRIES[0]:
        vopts = device.SgmViewOptions(0, 0, 0, 2, 0.95)
        return lib.smvs_sgm_depth_for_view_raw_photo(0, mp, W, H, 3, arr, nch, n_neighbors, 0, 16,
                                                     p1, p2, C.byref(vopts), f, dp, None, None,
                                                     n_witness, p, conf, vw)
    sopts = device.SgmSweepOptions(0, 0, 1, 0, 20, 0)
    rng = (C.c_float * 2)(1.0, 8.0)
    return lib.smvs_sgm_sweep_for_view_raw_photo(0, mp, W, H, 3, arr, nch, n_neighbors, 0, rng, 16,
                                                 p1, p2, C.byref(sopts), f, dp, None, None, None,
                                                 None, None, n_witness, p, conf, vw)


def test_photo_entries_exist_and_refuse_bad_arguments_without_a_gpu():
    """The three entries are exported and answer SMVS_ERR_INVALID with a message
    that names the argument -- before any device call, so also on a machine
    without a GPU -- to every argument outside the accepted set, in the order of
    include/smvs_hip.h: of two bad arguments the earlier one is named."""
    from smvs_amd import _capi
    lib = _hip_lib()
    for name in ENTRIES:
        assert name in _capi.declared_symbols() and hasattr(lib, name), name

    def refused(rc, word):
        assert rc == INVALID
        assert word in lib.smvs_last_error(), (word, lib.smvs_last_error())

    nan = float("nan")
    for entry in ENTRIES:
        refused(_call(lib, entry, null_photo=True), b"null photo")
        for radius in (-1, 4, 100):
            refused(_call(lib, entry, (radius, 2, 2, 0.49)), b"radius")
        for best_k in (-1, 4):           # three views in all
            refused(_call(lib, entry, (2, best_k, 2, 0.49)), b"best_k")
        for min_views in (-1, 4):
            refused(_call(lib, entry, (2, 2, min_views, 0.49)), b"min_views")
        for min_score in (-1.01, 1.01, nan):
            refused(_call(lib, entry, (2, 2, 2, min_score)), b"min_score")
        # the order: radius before best_k before min_views before min_score
        refused(_call(lib, entry, (4, 9, 9, nan)), b"radius")
        refused(_call(lib, entry, (2, 9, 9, nan)), b"best_k")
        refused(_call(lib, entry, (2, 2, 9, nan)), b"min_views")
        # the accepted corners pass the checks (and then need a device or run)
        for good in ((1, 0, 0, -1.0), (3, 3, 3, 1.0), (2, 1, 3, 0.0)):
            rc = _call(lib, entry, good)
            assert rc == 0 or (rc != INVALID and b"must" not in lib.smvs_last_error())
    for entry in ENTRIES[:2]:
        # the checks of the entry it extends come first
        refused(_call(lib, entry, (4, 2, 2, 0.49), filt=(100, 1, 0, 0.95)), b"uniqueness")
        # the witness count (best_k and min_views are checked against the total
        # before it: 0 passes for every count)
        refused(_call(lib, entry, (2, 0, 0, 0.49), n_witness=-1), b"n_witness")
        refused(_call(lib, entry, (2, 0, 0, 0.49), n_witness=15), b"n_witness")
        rc = _call(lib, entry, (2, 16, 16, 0.49), n_witness=14)
        assert rc == 0 or (rc != INVALID and b"must" not in lib.smvs_last_error())
        # radius 0 is off: a witness or an output of the test is an error
        refused(_call(lib, entry, (0, 2, 2, 0.49)), b"photo radius > 0")
        refused(_call(lib, entry, (0, 2, 2, 0.49), n_witness=0, views=False), b"photo radius > 0")
        refused(_call(lib, entry, (0, 2, 2, 0.49), n_witness=0, confidence=False),
                b"photo radius > 0")
        rc = _call(lib, entry, (0, 2, 2, 0.49), n_witness=0, confidence=False, views=False)
        assert rc == 0 or (rc != INVALID and b"must" not in lib.smvs_last_error())
        # a witness without an image, without a size, with a bad channel count
        refused(_call(lib, entry, bad_witness="image"), b"witness image")
        refused(_call(lib, entry, bad_witness="size"), b"witness image")
        for channels in (0, 2, 4):
            refused(_call(lib, entry, witness_channels=channels), b"channels (witness)")
        refused(_call(lib, entry, bad_witness="image", witness_channels=2), b"witness image")
    # the kernel alone: radius 0 is no test, the count, the pointers, the sizes
    refused(_call(lib, ENTRIES[2], (0, 2, 2, 0.49)), b"radius")
    refused(_call(lib, ENTRIES[2], (2, 0, 0, 0.49), n_neighbors=0, n_witness=0), b"n must")
    refused(_call(lib, ENTRIES[2], (2, 0, 0, 0.49), n_witness=15), b"n must")
    refused(_call(lib, ENTRIES[2], bad_witness="image"), b"witness image")
    refused(_call(lib, ENTRIES[2], bad_witness="size"), b"witness image")
    from smvs_amd import device
    u8p, fp = C.POINTER(C.c_uint8), C.POINTER(C.c_float)
    img = np.zeros((4, 5), np.uint8)
    a = np.ones((4, 5), F)
    arr = device._sgm_neighbors([dict(image=img, M_fwd=np.eye(3), t_fwd=[0, 0, 0], M_bwd=np.eye(3),
                                      t_bwd=[0, 0, 0], range_main=[1, 2], range_neighbor=[1, 2])],
                                [])
    opts = device.SgmPhotoOptions(1, 0, 0, 0.0)
    ip, ap = img.ctypes.data_as(u8p), a.ctypes.data_as(fp)

    def alone(main=ip, w=5, h=4, depth=ap, wit=arr, out=ap):
        return lib.smvs_sgm_photo_check(0, main, w, h, depth, wit, 1, C.byref(opts), out, None,
                                        None)
    for null in (dict(main=None), dict(depth=None), dict(wit=None), dict(out=None)):
        refused(alone(**null), b"null argument")
    for w, h in ((0, 4), (5, 0), (-1, 4), (65536, 32768)):
        refused(alone(w=w, h=h), b"map size")


def test_python_fronts_refuse_before_the_device():
    from smvs_amd import _capi, device
    main = np.full((H, W), 90, np.uint8)
    nb = dict(image=main, M_fwd=np.eye(3), t_fwd=[-6, 0, 0], M_bwd=np.eye(3), t_bwd=[6, 0, 0],
              range_main=[1, 8], range_neighbor=[1, 8])
    wit = dict(image=main, M_fwd=np.eye(3), t_fwd=[-6, 0, 0])
    depth = np.ones((H, W), F)
    with pytest.raises(_capi.SmvsError):
        device.sgm_photo_check(main, depth, [wit], radius=0)
    with pytest.raises(_capi.SmvsError):
        device.sgm_photo_check(main, depth, [wit], radius=4)
    with pytest.raises(_capi.SmvsError):
        device.sgm_photo_check(main, depth, [wit, wit], best_k=3)
    with pytest.raises(_capi.SmvsError):
        device.sgm_photo_check(main, depth, [wit, wit], min_score=float("nan"))
    with pytest.raises(_capi.SmvsError):
        device.sgm_photo_check(main, depth, [])
    with pytest.raises(_capi.SmvsError):
        device.sgm_photo_check(main, depth, [wit] * 17, best_k=0, min_views=0)
    with pytest.raises(ValueError):
        device.sgm_photo_check(main, depth[:-1], [wit])
    with pytest.raises(ValueError):
        device.sgm_photo_check(main, depth, [dict(wit, image=np.zeros((H, W, 3), np.uint8))])
    for front, args in ((device.sgm_depth_for_view, (main, [nb, nb])),
                        (device.sgm_sweep_for_view, (main, [nb, nb], (1, 8)))):
        with pytest.raises(_capi.SmvsError) as e:
            front(*args, num_steps=16, photo_radius=4)
        assert "radius" in str(e.value)
        with pytest.raises(_capi.SmvsError) as e:
            front(*args, num_steps=16, photo_radius=2, photo_min_views=3)
        assert "min_views" in str(e.value)
        with pytest.raises(_capi.SmvsError) as e:
            front(*args, num_steps=16, photo_radius=2, photo_min_score=1.5)
        assert "min_score" in str(e.value)
        # off is off: witnesses, or a changed option that asks for nothing, are
        # never silently ignored
        with pytest.raises(_capi.SmvsError) as e:
            front(*args, num_steps=16, witnesses=[wit])
        assert "photo radius > 0" in str(e.value)
        with pytest.raises(_capi.SmvsError) as e:
            front(*args, num_steps=16, photo_radius=2, witnesses=[wit] * 15)
        assert "n_witness" in str(e.value)


def test_host_and_python_options_default_to_off():
    """SGMStereo::Options and ReconSettings hold (0, 2, 2, 0.49, -1) when
    default-constructed, the Python fronts default to the same -- off -- and call
    the entries without the test then, and a value outside the accepted set is an
    error in the host entries before anything runs."""
    from smvs_amd import _capi, device, host, synth
    hlib = host.load()
    hlib.smvs_host_last_error.restype = C.c_char_p
    for name in ("smvs_host_sgm_depth_photo", "smvs_host_reconstruct_scene_photo",
                 "smvs_host_sgm_photo_defaults"):
        assert hasattr(hlib, name), name
    ints = (C.c_int * 8)(*([7] * 8))
    scores = (C.c_float * 2)(7.0, 7.0)
    assert hlib.smvs_host_sgm_photo_defaults(ints, scores) == 0
    assert list(ints) == [0, 2, 2, -1] * 2 and list(scores) == [F(0.49)] * 2
    assert hlib.smvs_host_sgm_photo_defaults(None, scores) != 0
    assert device.SGM_PHOTO_DEFAULTS == (0, 2, 2, 0.49)
    four = dict(photo_radius=0, photo_best_k=2, photo_min_views=2, photo_min_score=0.49)
    want = {device.sgm_depth_for_view: dict(four, witnesses=None),
            device.sgm_sweep_for_view: dict(four, witnesses=None),
            device.sgm_photo_check: dict(radius=2, best_k=2, min_views=2, min_score=0.49),
            host.sgm_depth: dict(four, photo_witnesses=-1),
            host.reconstruct_scene: dict({"sgm_" + k: v for k, v in four.items()},
                                         sgm_photo_witnesses=-1)}
    for fn, defaults in want.items():
        for key, value in defaults.items():
            got = inspect.signature(fn).parameters[key].default
            assert got == value and type(got) is type(value), (fn, key)
    assert [f[0] for f in device.SgmPhotoOptions._fields_] == [
        "radius", "best_k", "min_views", "min_score"]
    assert C.sizeof(device.SgmPhotoOptions) == 16
    assert device._sgm_photo(0, 2, 2, 0.49, None) is None
    assert device._sgm_photo(0, 2, 2, 0.49, []) is None
    assert device._sgm_photo(2, 2, 2, 0.49, None) is not None
    assert device._sgm_photo(0, 2, 2, 0.49, [dict()]) is not None
    assert device._sgm_photo(0, 2, 2, 0.5, None) is not None
    assert [f[0] for f in host.SgmPhoto._fields_] == ["radius", "best_k", "min_views",
                                                      "min_score", "witnesses"]
    assert C.sizeof(host.SgmPhoto) == 20
    inputs = synth.pipeline_inputs("plane", 48, 32, 3, n_features=50)
    bad_options = (dict(radius=4), dict(radius=-1), dict(best_k=-1), dict(best_k=17),
                   dict(min_views=-1), dict(min_views=17), dict(min_score=1.5),
                   dict(min_score=-1.5), dict(min_score=float("nan")), dict(witnesses=-2),
                   dict(witnesses=17))
    for bad in bad_options:
        with pytest.raises(_capi.SmvsError) as e:
            host.sgm_depth(inputs, 1, **{"photo_" + k: v for k, v in bad.items()})
        assert "sgm_photo_radius" in str(e.value), bad
    st = host.ReconSettings(b"undistorted", 1.0, 2, 0, 1, 0, 0, 0, 0.0, 0.0, 1, 6, 3, 0, 1, 2,
                            -1, 1700000)
    n = C.c_int(0)

    def scene(**photo):
        p = host.SgmPhoto(**dict(dict(radius=2, best_k=2, min_views=2, min_score=0.49,
                                      witnesses=-1), **photo))
        return hlib.smvs_host_reconstruct_scene_photo(
            b"/nonexistent", C.byref(st), C.c_uint(0), C.c_int(128), C.c_int(0), C.c_int(2),
            C.c_int(0), C.c_float(0.95), C.c_int(2), None, None, C.byref(p), None, 0, None, 0,
            C.byref(n), None, None, None)
    for bad in bad_options:
        assert scene(**bad) != 0 and b"sgm_photo_radius" in hlib.smvs_host_last_error(), bad
    # accepted: the call gets as far as the scene, which is not there
    assert scene(radius=3, best_k=16, min_views=0, min_score=-1.0, witnesses=16) != 0
    assert b"sgm_" not in hlib.smvs_host_last_error()
