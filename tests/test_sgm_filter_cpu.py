"""CPU checks of the two opt-in filters of the SGM front end (DESIGN.md section
3.6, "uniqueness test and speckle removal"; include/smvs_hip.h, "Two single-run
rejections"): the numpy restatement tests/sgm_filter_ref.py on tables worked out
by hand and on the edges of both definitions, the argument checks of the six new
entries, which need no GPU, and the defaults of the host mirror and the Python
fronts."""
import ctypes as C
import inspect

import numpy as np
import pytest

import sgm_filter_ref as ref             # tests/sgm_filter_ref.py
import sgm_subplane_ref as subplane_ref  # tests/sgm_subplane_ref.py

F = np.float32
INVALID = -1


# ------------------------------------------------------------------ uniqueness
def _one_pixel(S, uniq, window):
    S = np.asarray(S, np.uint16)[None, None, :]
    i = np.array([[int(np.argmin(S[0, 0]))]], np.int32)     # the first minimum
    rejected, runner, none = ref.uniqueness(S, i, uniq, window)
    return bool(rejected[0, 0]), int(runner[0, 0]), bool(none[0, 0])


def test_uniqueness_by_hand():
    """Winner plane 2 (S = 90); window 1 leaves the planes 0, 4 and 5."""
    S = [120, 91, 90, 91, 100, 130]
    # r = 100: 100 * 90 = 9000 < 90 * 100 = 9000 is false -- exactly at the bound
    # passes, the comparison is strict
    assert _one_pixel(S, 10, 1) == (False, 100, False)
    # one less fails it: r = 99, 8910 < 9000
    assert _one_pixel([120, 91, 90, 91, 99, 130], 10, 1) == (True, 99, False)
    # uniqueness 0 rejects nothing (r >= b always: b is the minimum)
    assert _one_pixel([90, 91, 90, 90, 90, 90], 0, 1) == (False, 90, False)
    # window 2 leaves plane 5; window 3 leaves nothing: the pixel passes, 65535
    assert _one_pixel(S, 10, 2) == (False, 130, False)
    assert _one_pixel(S, 99, 2) == (True, 130, False)       # 130 < 9000
    assert _one_pixel(S, 99, 3) == (False, 65535, True)
    assert _one_pixel(S, 99, 256) == (False, 65535, True)
    # the first minimum is the winner: the second one, three planes on, competes
    assert _one_pixel([50, 60, 70, 50], 1, 1) == (True, 50, False)
    # the neighbours inside the window never compete, however cheap
    assert _one_pixel([90, 90, 90, 200], 50, 2) == (False, 200, False)
    # a winner at the last plane: competitors on one side only
    assert _one_pixel([95, 200, 200, 90], 10, 1) == (True, 95, False)
    assert _one_pixel([200, 95, 200, 90], 10, 1)[1] == 95
    # sums at the top of u16 stay inside 32 bits
    assert _one_pixel([65535, 0, 0, 65535], 1, 1) == (False, 65535, False)
    assert _one_pixel([65000, 65001, 65535, 65535], 1, 1) == (True, 65535, False)


def test_uniqueness_keeps_argmin_and_every_other_bit():
    depth = np.array([[1.5, 2.5], [0.0, 3.5]], F)
    rejected = np.array([[True, False], [True, False]])
    out = ref.apply_uniqueness(depth, rejected)
    assert out.dtype == F and out.tolist() == [[0.0, 2.5], [0.0, 3.5]]


def test_uniqueness_without_a_competitor_on_the_pair(oracle):
    """The (8 planes, 3 .. 12) run of the pair of tests/sgm_subplane_ref.py: at
    window 4 the winners 3 and 4 have no competitor, at window 8 no pixel has;
    such a pixel passes at any uniqueness."""
    main, nbr, M, t = subplane_ref.scene_pair()
    depths = oracle.sgm_depths(3, 12, 8)
    S = oracle.sgm_aggregate(oracle.sgm_cost_volume(main, nbr, M, t, depths), 6, 96)
    plane, i = oracle.sgm_depth_from_volume(S, main, depths)
    v = plane > 0
    rejected, runner, none = ref.uniqueness(S, i, 99, 4)
    print("valid %d, without a competitor at window 4: %d" % (v.sum(), (none & v).sum()))
    assert (none & v).sum() == 468 and v.sum() == 3915
    assert np.array_equal(none, (i == 3) | (i == 4))
    assert not rejected[none].any() and (runner[none] == 65535).all()
    assert rejected[v & ~none].any()
    rejected, runner, none = ref.uniqueness(S, i, 99, 8)
    assert none.all() and not rejected.any() and (runner == 65535).all()


# --------------------------------------------------------------------- speckles
def test_speckles_by_hand():
    """Three components under ratio 0.9: the five 1.0s (joined round the
    corner), the two 2.0s, the lone 4.0."""
    a = np.array([[1.0, 1.0, 0.0, 2.0],
                  [0.0, 1.0, 0.0, 2.0],
                  [4.0, 1.0, 1.0, 0.0]], F)
    size = ref.component_sizes(a, 0.9)
    assert size.dtype == np.uint32
    assert size.tolist() == [[5, 5, 0, 2], [0, 5, 0, 2], [1, 5, 5, 0]]
    out, size2 = ref.filter_speckles(a, 3, 0.9)
    assert np.array_equal(size2, size)
    assert out.tolist() == [[1, 1, 0, 0], [0, 1, 0, 0], [0, 1, 1, 0]]
    # sizes 0 and 1 remove nothing; a size above every component removes all
    for off in (0, 1):
        assert ref.filter_speckles(a, off, 0.9)[0].tobytes() == a.tobytes()
    assert not ref.filter_speckles(a, 6, 0.9)[0].any()
    # diagonal neighbours are not neighbours
    d = np.array([[1.0, 0.0], [0.0, 1.0]], F)
    assert ref.component_sizes(d, 0.0).tolist() == [[1, 0], [0, 1]]
    # ratio 0 links every pair of valid neighbours, ratio 1 only equal ones
    e = np.array([[1.0, 100.0, 100.0]], F)
    assert ref.component_sizes(e, 0.0).tolist() == [[3, 3, 3]]
    assert ref.component_sizes(e, 1.0).tolist() == [[1, 2, 2]]


def test_speckle_link_at_the_threshold():
    """1.0, 0.5, 0.25 at ratio 0.5: the quotients are exactly the threshold and
    link (>=); a pair just below it does not."""
    row = np.array([[1.0, 0.5, 0.25]], F)
    assert ref.component_sizes(row, 0.5).tolist() == [[3, 3, 3]]
    below = np.nextafter(F(0.5), F(0))
    row = np.array([[1.0, below, 0.25]], F)
    # 1.0 | below: the quotient is below 0.5; below | 0.25: above it
    assert ref.component_sizes(row, 0.5).tolist() == [[1, 2, 2]]
    column = np.array([[1.0], [0.5], [below / 2]], F)
    assert ref.component_sizes(column, 0.5).tolist() == [[2], [2], [1]]


def test_speckle_components_are_the_transitive_closure():
    """1.0, 1.04, 1.08 at ratio 0.95: one component although 1.0 / 1.08 < 0.95
    (the consensus's star would not join the ends)."""
    chain = np.array([[1.0, 1.04, 1.08]], F)
    assert F(1.0) / F(1.08) < F(0.95) <= F(1.0) / F(1.04)
    assert F(1.04) / F(1.08) >= F(0.95)
    assert ref.component_sizes(chain, 0.95).tolist() == [[3, 3, 3]]
    assert ref.component_sizes(np.array([[1.0, 0.0, 1.08]], F), 0.95).tolist() == [[1, 0, 1]]


@pytest.mark.parametrize("k", [2, 5, 40])
def test_speckle_size_is_a_strict_bound(k):
    """Two components of k and k - 1 pixels at speckle_size k: one kept, one
    removed."""
    a = np.zeros((3, k + 2), F)
    a[0, :k] = 2.0
    a[2, :k - 1] = 2.0
    out, size = ref.filter_speckles(a, k, 0.95)
    assert size[0, :k].tolist() == [k] * k and size[2, :k - 1].tolist() == [k - 1] * (k - 1)
    assert (out[0, :k] == 2.0).all() and not out[2].any() and not out[1].any()


def test_pixels_that_are_not_valid_keep_their_bits():
    """A NaN, a negative, a zero and a negative zero are in no component: size 0,
    bits kept, and they separate their neighbours."""
    a = np.array([[1.0, 0.0, 1.0, -2.0, 1.0, 0.0, 1.0, -0.0, 1.0, np.inf, np.inf]], F)
    a.view(np.uint32)[0, 1] = 0x7FC12345        # a NaN with a payload
    assert np.isnan(a[0, 1])
    out, size = ref.filter_speckles(a, 2, 0.5)
    # (an infinite depth is valid; 1 / inf is below the ratio and inf / inf is no
    # number: it links with nothing)
    assert size.tolist() == [[1, 0, 1, 0, 1, 0, 1, 0, 1, 1, 1]]
    want = a.copy()
    want[0, [0, 2, 4, 6, 8, 9, 10]] = 0
    assert out.tobytes() == want.tobytes()
    assert out.view(np.uint32)[0, 1] == 0x7FC12345 and out.view(np.uint32)[0, 7] == 0x80000000
    assert out[0, 3] == -2.0


# ------------------------------------------------------------------ the entries
def _hip_lib():
    from smvs_amd import _capi
    lib = _capi.load()
    lib.smvs_last_error.restype = C.c_char_p
    return lib


W, H = 24, 16
ENTRIES = ("smvs_sgm_run_filtered", "smvs_sgm_depth_for_view_filtered",
           "smvs_sgm_depth_for_view_raw_filtered", "smvs_sgm_sweep_for_view_filtered",
           "smvs_sgm_sweep_for_view_raw_filtered", "smvs_sgm_filter_speckles")


def _call(lib, entry, filt, runner_up=False):
    """one of the five entries that take the filter options, on a small image"""
    from smvs_amd import device
    u8p, fp, u16p = C.POINTER(C.c_uint8), C.POINTER(C.c_float), C.POINTER(C.c_uint16)
    raw = "raw" in entry
    main = np.full((H, W, 3) if raw else (H, W), 90, np.uint8)
    nb = dict(image=main, M_fwd=np.eye(3), t_fwd=[-6, 0, 0], M_bwd=np.eye(3), t_bwd=[6, 0, 0],
              range_main=[1, 8], range_neighbor=[1, 8])
    keep = []
    arr = device._sgm_neighbors([nb] * 2, keep)
    nch = (C.c_int * 2)(3, 3)
    depth = np.zeros((H, W), F)
    runner = np.zeros((H, W), np.uint16).ctypes.data_as(u16p) if runner_up else None
    f = C.byref(filt) if filt is not None else None
    p1, p2 = C.c_uint16(6), C.c_uint16(96)
    mp, dp = main.ctypes.data_as(u8p), depth.ctypes.data_as(fp)
    if entry == "smvs_sgm_run_filtered":
        opts = device.SgmOptions(0, 0)
        M = np.eye(3, dtype=F).reshape(9)
        t = np.array([-6, 0, 0], F)
        return lib.smvs_sgm_run_filtered(0, mp, W, H, mp, W, H, M.ctypes.data_as(fp),
                                         t.ctypes.data_as(fp), C.c_float(1), C.c_float(8), 16,
                                         p1, p2, C.byref(opts), f, dp, None, None, None, runner)
    if entry.startswith("smvs_sgm_depth_for_view"):
        vopts = device.SgmViewOptions(0, 0, 0, 2, 0.95)
        if raw:
            return lib.smvs_sgm_depth_for_view_raw_filtered(0, mp, W, H, 3, arr, nch, 2, 0, 16,
                                                            p1, p2, C.byref(vopts), f, dp, None,
                                                            None)
        return lib.smvs_sgm_depth_for_view_filtered(0, mp, W, H, arr, 2, 16, p1, p2,
                                                    C.byref(vopts), f, dp, None, None)
    sopts = device.SgmSweepOptions(0, 0, 1, 0, 20, 0)
    rng = (C.c_float * 2)(1.0, 8.0)
    if raw:
        return lib.smvs_sgm_sweep_for_view_raw_filtered(0, mp, W, H, 3, arr, nch, 2, 0, rng, 16,
                                                        p1, p2, C.byref(sopts), f, dp, None)
    return lib.smvs_sgm_sweep_for_view_filtered(0, mp, W, H, arr, 2, rng, 16, p1, p2,
                                                C.byref(sopts), f, dp, None, None, None, None,
                                                runner)


def test_filtered_entries_exist_and_refuse_bad_arguments_without_a_gpu():
    """The six entries are exported and answer SMVS_ERR_INVALID with a message
    that names the argument -- before any device call, so also on a machine
    without a GPU -- to every filter option outside the accepted set."""
    from smvs_amd import _capi, device
    lib = _hip_lib()
    for name in ENTRIES:
        assert name in _capi.declared_symbols() and hasattr(lib, name), name

    def refused(rc, word):
        assert rc == INVALID
        assert word in lib.smvs_last_error(), (word, lib.smvs_last_error())

    nan = float("nan")
    for entry in ENTRIES[:5]:
        refused(_call(lib, entry, None), b"null filter")
        for uniq in (-1, 100, 1000):
            refused(_call(lib, entry, device.SgmFilterOptions(uniq, 1, 0, 0.95)), b"uniqueness")
        for window in (0, -1, 257):
            refused(_call(lib, entry, device.SgmFilterOptions(10, window, 0, 0.95)),
                    b"uniqueness_window")
        refused(_call(lib, entry, device.SgmFilterOptions(10, 1, -1, 0.95)), b"speckle_size")
        for ratio in (-0.01, 1.01, nan):
            refused(_call(lib, entry, device.SgmFilterOptions(10, 1, 0, ratio)), b"speckle_ratio")
        # the accepted corners pass the checks (and then need a device or run)
        for good in ((0, 1, 0, 0.0), (99, 256, 1, 1.0), (0, 256, 0, 0.5)):
            rc = _call(lib, entry, device.SgmFilterOptions(*good))
            assert rc == 0 or (rc != INVALID and b"must" not in lib.smvs_last_error())
    # the speckle fields on the run entry; runner_up without the test
    refused(_call(lib, ENTRIES[0], device.SgmFilterOptions(10, 1, 2, 0.95)), b"speckle")
    refused(_call(lib, ENTRIES[0], device.SgmFilterOptions(0, 1, 0, 0.95), runner_up=True),
            b"runner_up")
    refused(_call(lib, ENTRIES[3], device.SgmFilterOptions(0, 1, 0, 0.95), runner_up=True),
            b"runner_up")
    # the options of the entries they extend are still checked
    fp = C.POINTER(C.c_float)
    a = np.ones((4, 5), F)
    ap = a.ctypes.data_as(fp)

    def speckles(depth=ap, w=5, h=4, size=3, ratio=0.95, out=ap):
        return lib.smvs_sgm_filter_speckles(0, depth, w, h, size, C.c_float(ratio), out, None)
    refused(speckles(size=-1), b"speckle_size")
    for ratio in (-0.5, 1.5, nan):
        refused(speckles(ratio=ratio), b"speckle_ratio")
    refused(speckles(depth=None), b"null")
    refused(speckles(out=None), b"null")
    for w, h in ((0, 4), (5, 0), (-1, 4), (65536, 32768)):
        refused(speckles(w=w, h=h), b"map size")


def test_python_fronts_refuse_before_the_device():
    from smvs_amd import _capi, device
    main = np.full((H, W), 90, np.uint8)
    nb = dict(image=main, M_fwd=np.eye(3), t_fwd=[-6, 0, 0], M_bwd=np.eye(3), t_bwd=[6, 0, 0],
              range_main=[1, 8], range_neighbor=[1, 8])
    with pytest.raises(_capi.SmvsError):
        device.sgm_run(main, main, np.eye(3), [-6, 0, 0], 1, 8, 16, uniqueness=100)
    with pytest.raises(_capi.SmvsError):
        device.sgm_run(main, main, np.eye(3), [-6, 0, 0], 1, 8, 16, uniqueness_window=0)
    with pytest.raises(_capi.SmvsError):
        device.sgm_depth_for_view(main, [nb, nb], num_steps=16, speckle_size=-1)
    with pytest.raises(_capi.SmvsError):
        device.sgm_depth_for_view(main, [nb, nb], num_steps=16, consensus=True, speckle_ratio=2.0)
    with pytest.raises(_capi.SmvsError):
        device.sgm_sweep_for_view(main, [nb, nb], (1, 8), num_steps=16, uniqueness_window=300)
    with pytest.raises(_capi.SmvsError):
        device.sgm_filter_speckles(np.ones((4, 5), F), -1, 0.95)
    with pytest.raises(ValueError):
        device.sgm_filter_speckles(np.ones(5, F), 3, 0.95)


def test_host_and_python_options_default_to_off():
    """SGMStereo::Options and ReconSettings hold (0, 1, 0, 0.95) when
    default-constructed, the Python fronts default to the same, and a value
    outside the accepted set is an error in the host entries before anything
    runs."""
    from smvs_amd import _capi, device, host, synth
    hlib = host.load()
    hlib.smvs_host_last_error.restype = C.c_char_p
    for name in ("smvs_host_sgm_depth_filtered", "smvs_host_reconstruct_scene_filtered",
                 "smvs_host_sgm_filter_defaults"):
        assert hasattr(hlib, name), name
    ints = (C.c_int * 6)(*([7] * 6))
    ratios = (C.c_float * 2)(7.0, 7.0)
    assert hlib.smvs_host_sgm_filter_defaults(ints, ratios) == 0
    assert list(ints) == [0, 1, 0] * 2 and list(ratios) == [F(0.95)] * 2
    assert hlib.smvs_host_sgm_filter_defaults(None, ratios) != 0
    assert device.SGM_FILTER_DEFAULTS == (0, 1, 0, 0.95)
    four = dict(uniqueness=0, uniqueness_window=1, speckle_size=0, speckle_ratio=0.95)
    want = {device.sgm_run: dict(uniqueness=0, uniqueness_window=1),
            device.sgm_depth_for_view: four, device.sgm_sweep_for_view: four,
            device.sgm_filter_speckles: dict(speckle_ratio=0.95),
            host.sgm_depth: four,
            host.reconstruct_scene: {"sgm_" + k: v for k, v in four.items()}}
    for fn, defaults in want.items():
        for key, value in defaults.items():
            got = inspect.signature(fn).parameters[key].default
            assert got == value and type(got) is type(value), (fn, key)
    assert [f[0] for f in device.SgmFilterOptions._fields_] == [
        "uniqueness", "uniqueness_window", "speckle_size", "speckle_ratio"]
    assert [f[0] for f in host.SgmFilter._fields_] == [f[0] for f in
                                                       device.SgmFilterOptions._fields_]
    assert C.sizeof(device.SgmFilterOptions) == 16 and C.sizeof(host.SgmFilter) == 16
    # the Python fronts call the entries without the filters at the defaults
    assert device._sgm_filter(0, 1, 0, 0.95) is None
    assert device._sgm_filter(0, 1, 2, 0.95) is not None
    inputs = synth.pipeline_inputs("plane", 48, 32, 3, n_features=50)
    for bad in (dict(uniqueness=100), dict(uniqueness=-1), dict(uniqueness_window=0),
                dict(uniqueness_window=257), dict(speckle_size=-1), dict(speckle_ratio=1.5),
                dict(speckle_ratio=float("nan"))):
        with pytest.raises(_capi.SmvsError) as e:
            host.sgm_depth(inputs, 1, **bad)
        assert "sgm_uniqueness" in str(e.value), bad
    st = host.ReconSettings(b"undistorted", 1.0, 2, 0, 1, 0, 0, 0, 0.0, 0.0, 1, 6, 3, 0, 1, 2,
                            -1, 1700000)
    n = C.c_int(0)

    def scene(filt):
        f = host.SgmFilter(*filt)
        return hlib.smvs_host_reconstruct_scene_filtered(
            b"/nonexistent", C.byref(st), C.c_uint(0), C.c_int(128), C.c_int(0), C.c_int(2),
            C.c_int(0), C.c_float(0.95), C.c_int(2), None, C.byref(f), None, 0, None, 0,
            C.byref(n), None, None, None)
    for filt in ((100, 1, 0, 0.95), (10, 0, 0, 0.95), (10, 1, -1, 0.95), (10, 1, 0, -0.1)):
        assert scene(filt) != 0 and b"sgm_uniqueness" in hlib.smvs_host_last_error(), filt
    # accepted: the call gets as far as the scene, which is not there
    assert scene((99, 256, 200, 1.0)) != 0
    assert b"sgm_" not in hlib.smvs_host_last_error()
