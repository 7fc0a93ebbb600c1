"""CPU checks of the consensus merge of the SGM front end (DESIGN.md section
3.6, "n-neighbour consensus"; SMVS_SGM_MERGE_CONSENSUS of include/smvs_hip.h):
the numpy restatement tests/sgm_merge_ref.py against the reference's
two-neighbour merge on the oracle's checked maps and against a hand-written
table, and the argument checks of the three new entries, which need no GPU."""
import ctypes as C
import inspect

import numpy as np
import pytest

import sgm_merge_ref as ref  # tests/sgm_merge_ref.py

F = np.float32
INVALID = -1


# ------------------------------------------------- the reference's merge, n = 2
def test_two_maps_at_ratio_0_are_the_reference_merge_bit_for_bit(oracle):
    """1. On the oracle's two checked maps of the sphere scene the restatement
    with (agree_ratio 0, min_agree 1) is the reference's merge and is
    oracle.sgm_depth_for_view; one map alone gives itself."""
    from smvs_amd import host, synth
    inputs = synth.pipeline_inputs("sphere", 384, 256, 3, flen=1.2)
    imgs = [host.sgm_image(inputs, k, 1) for k in range(3)]
    small = dict(inputs, images=imgs)

    def run(a, b, M, t, rng):
        depths = oracle.sgm_depths(rng[0], rng[1], 128)
        S = oracle.sgm_aggregate(oracle.sgm_cost_volume(a, b, M, t, depths), 6, 96)
        return oracle.sgm_depth_from_volume(S, a, depths)[0]
    checked = []
    for k in (1, 2):
        Mf, tf = host.view_reprojection(small, 0, k)
        Mb, tb = host.view_reprojection(small, k, 0)
        fwd = run(imgs[0], imgs[k], Mf, tf, host.depth_range(inputs, 0))
        bwd = run(imgs[k], imgs[0], Mb, tb, host.depth_range(inputs, k))
        checked.append(oracle.sgm_lr_check(fwd, bwd, Mf, tf))
    stack = np.stack(checked)
    both = (stack[0] != 0) & (stack[1] != 0)
    only = (stack[0] != 0) ^ (stack[1] != 0)
    print("both valid %d, one valid %d, none %d of %d; the two differ at %d of the first"
          % (both.sum(), only.sum(), (~both & ~only).sum(), both.size,
             (both & (stack[0] != stack[1])).sum()))
    assert both.sum() >= 1 and only.sum() >= 1 and (both & (stack[0] != stack[1])).sum() >= 1
    merged, support, best = ref.consensus(stack, 0.0, 1)
    assert merged.dtype == F and support.dtype == np.uint8
    assert np.array_equal(merged, ref.reference_merge(stack[0], stack[1]))
    assert np.array_equal(merged, oracle.sgm_depth_for_view(inputs, sgm_scale=1))
    assert np.array_equal(support, (stack != 0).sum(axis=0))
    for k in (0, 1):
        for ratio in (0.0, 0.95, 1.0):
            alone, s1, _ = ref.consensus(stack[k:k + 1], ratio, 1)
            assert np.array_equal(alone, stack[k])
            assert np.array_equal(s1, stack[k] != 0)


# ------------------------------------------------------------------ the table
# (c[0 .. n-1], agree_ratio, min_agree) -> (out, support, best); every number
# is a float32 value, so the sums and quotients below are exact
TABLE = [
    # a tie of two clusters keeps the lower k
    ("tie", [1.0, 1.0, 2.0, 2.0], 0.9, 1, 1.0, 2, 0),
    ("tie, second cluster first", [2.0, 1.0, 2.0, 1.0], 0.9, 1, 2.0, 2, 0),
    ("tie of singles", [4.0, 2.0], 0.9, 1, 4.0, 1, 0),
    # a ~ b ~ c with a !~ c (1 / 1.125 = 0.889 < 0.9): b's star of three wins
    # over a's of two; (1 + 1.0625 + 1.125) / 3 = 1.0625
    ("chain", [1.0, 1.0625, 1.125], 0.9, 1, 1.0625, 3, 1),
    ("chain, b last", [1.0, 1.125, 1.0625], 0.9, 1, 1.0625, 3, 2),
    # not a transitive closure: without b in the middle a and c stand alone
    ("no chain", [1.0, 1.125], 0.9, 1, 1.0, 1, 0),
    # a ratio exactly equal to agree_ratio counts (3 / 4 and 1 / 2 are exact)
    ("equal ratio", [3.0, 4.0], 0.75, 2, 3.5, 2, 0),
    ("equal ratio", [1.0, 0.0, 2.0], 0.5, 2, 1.5, 2, 0),
    ("just above", [3.0, 4.0], 0.7500001, 1, 3.0, 1, 0),
    ("identical at 1", [2.5, 2.5, 2.5], 1.0, 3, 2.5, 3, 0),
    # min_agree above the best count
    ("min_agree", [1.0, 2.0, 0.0], 0.9, 2, 0.0, 1, 0),
    ("min_agree", [1.0, 1.0, 3.0], 0.9, 3, 0.0, 2, 0),
    ("min_agree met", [1.0, 1.0, 3.0], 0.9, 2, 1.0, 2, 0),
    # all zero
    ("all zero", [0.0, 0.0, 0.0], 0.0, 1, 0.0, 0, 0),
    ("all zero", [0.0], 0.95, 1, 0.0, 0, 0),
    # a single valid map gives itself, whatever the ratio
    ("single", [0.0, 0.0, 5.5], 1.0, 1, 5.5, 1, 2),
    ("single", [0.0, 0.0, 5.5], 0.0, 1, 5.5, 1, 2),
    ("single", [7.25], 0.95, 1, 7.25, 1, 0),
    # the winner is not the first valid map; a valid map stays outside the star
    ("second wins", [1.0, 2.0, 2.0], 0.9, 1, 2.0, 2, 1),
    ("zeros between", [0.0, 3.0, 0.0, 1.0, 3.0, 3.0], 0.95, 2, 3.0, 3, 1),
    # ratio 0: every valid map supports every other one; (1 + 2 + 6) / 3 = 3
    ("ratio 0", [1.0, 2.0, 0.0, 6.0], 0.0, 1, 3.0, 3, 0),
]


@pytest.mark.parametrize("row", TABLE, ids=["%02d-%s" % (i, r[0].replace(" ", "-").replace(",", "")) for i, r in enumerate(TABLE)])
def test_restatement_on_the_table(row):
    """2. hand-written pixel vectors with their outputs spelt out"""
    _, c, ratio, min_agree, out, support, best = row
    stack = np.array(c, F).reshape(len(c), 1)
    merged, sup, b = ref.consensus(stack, ratio, min_agree)
    assert merged.dtype == F
    assert merged[0] == F(out) and int(sup[0]) == support and int(b[0]) == best


def test_table_as_one_image_per_parameter_pair():
    """2. the rows that share (n, agree_ratio, min_agree) as pixels of one call"""
    groups = {}
    for row in TABLE:
        groups.setdefault((len(row[1]), row[2], row[3]), []).append(row)
    assert any(len(g) > 1 for g in groups.values())
    for (n, ratio, min_agree), rows in groups.items():
        stack = np.array([r[1] for r in rows], F).T.copy()
        merged, sup, b = ref.consensus(stack, ratio, min_agree)
        assert np.array_equal(merged, np.array([r[4] for r in rows], F))
        assert [int(x) for x in sup] == [r[5] for r in rows]
        assert [int(x) for x in b] == [r[6] for r in rows]


# ------------------------------------------------------------- the new entries
def _hip_lib():
    from smvs_amd import _capi
    return _capi.load()


def _view_options(p2_mode=0, winner=0, merge=1, min_agree=2, agree_ratio=0.95):
    from smvs_amd.device import SgmViewOptions
    return SgmViewOptions(p2_mode, winner, merge, min_agree, agree_ratio)


def _neighbors(n, main):
    from smvs_amd.device import SgmNeighbor
    h, w = main.shape
    arr = (SgmNeighbor * max(n, 1))()
    for k in range(n):
        arr[k].image = main.ctypes.data_as(C.POINTER(C.c_uint8))
        arr[k].width, arr[k].height = w, h
        for i in range(9):
            arr[k].M_fwd[i] = arr[k].M_bwd[i] = float(i % 4 == 0)
        arr[k].t_fwd[0], arr[k].t_bwd[0] = -6.0, 6.0
        arr[k].range_main[0] = arr[k].range_neighbor[0] = 1.0
        arr[k].range_main[1] = arr[k].range_neighbor[1] = 8.0
    return arr


def _view_merge(lib, opts, raw, n=2, num_steps=16):
    w, h = 24, 16
    main = np.full((h, w), 90, np.uint8)
    arr = _neighbors(n, main)
    depth = np.zeros((h, w), np.float32)
    u8, fp = C.POINTER(C.c_uint8), C.POINTER(C.c_float)
    po = C.byref(opts) if opts is not None else None
    if raw:
        ch = (C.c_int * max(n, 1))(*([1] * max(n, 1)))
        return lib.smvs_sgm_depth_for_view_raw_merge(
            0, main.ctypes.data_as(u8), w, h, 1, arr, ch, n, 0, num_steps, C.c_uint16(6),
            C.c_uint16(96), po, depth.ctypes.data_as(fp), None, None)
    return lib.smvs_sgm_depth_for_view_merge(
        0, main.ctypes.data_as(u8), w, h, arr, n, num_steps, C.c_uint16(6), C.c_uint16(96), po,
        depth.ctypes.data_as(fp), None, None)


def _check_merge(lib, opts, n=2):
    from smvs_amd.device import SgmCheckNeighbor
    w, h = 24, 16
    fwd = np.full((max(n, 1), h, w), 2.0, np.float32)
    bwd = np.full((h, w), 2.0, np.float32)
    arr = (SgmCheckNeighbor * max(n, 1))()
    fp = C.POINTER(C.c_float)
    for k in range(n):
        arr[k].bwd = bwd.ctypes.data_as(fp)
        arr[k].width, arr[k].height = w, h
        for i in range(9):
            arr[k].M_fwd[i] = float(i % 4 == 0)
    merged = np.zeros((h, w), np.float32)
    return lib.smvs_sgm_check_merge(0, fwd.ctypes.data_as(fp), w, h, arr, n,
                                    C.byref(opts) if opts is not None else None,
                                    merged.ctypes.data_as(fp), None, None)


def test_merge_entries_exist_and_refuse_bad_arguments_without_a_gpu():
    """3. smvs_sgm_depth_for_view_merge, ..._raw_merge and smvs_sgm_check_merge
    are exported and answer SMVS_ERR_INVALID -- before any device call, so also
    on a machine without a GPU -- to NULL options, an unknown merge, 0 and 17
    neighbours, three neighbours with the reference's merge, an agree_ratio of
    -0.1, 1.5 and NaN, and a min_agree of 0 (and 17).  The `_opts` entry still
    refuses three neighbours."""
    from smvs_amd import _capi
    from smvs_amd.device import SgmNeighbor, SgmOptions
    lib = _hip_lib()
    for name in ("smvs_sgm_depth_for_view_merge", "smvs_sgm_depth_for_view_raw_merge",
                 "smvs_sgm_check_merge"):
        assert name in _capi.declared_symbols() and hasattr(lib, name), name
    calls = [lambda o, **kw: _view_merge(lib, o, raw=False, **kw),
             lambda o, **kw: _view_merge(lib, o, raw=True, **kw),
             lambda o, **kw: _check_merge(lib, o, **kw)]
    for i, call in enumerate(calls):
        assert call(None) == INVALID
        assert b"options" in lib.smvs_last_error()
        for merge in (2, -1, 7):
            assert call(_view_options(merge=merge)) == INVALID
            assert b"merge" in lib.smvs_last_error()
        for n in (0, 17, -1):
            assert call(_view_options(), n=n) == INVALID
            assert b"SMVS_MAX_SUBS" in lib.smvs_last_error()
        assert call(_view_options(merge=0), n=3) == INVALID
        assert (b"one or two neighbours" if i < 2 else b"consensus") in lib.smvs_last_error()
        for ratio in (-0.1, 1.5, float("nan"), float("inf")):
            assert call(_view_options(agree_ratio=ratio)) == INVALID
            assert b"agree_ratio" in lib.smvs_last_error()
        for min_agree in (0, 17, -2):
            assert call(_view_options(min_agree=min_agree)) == INVALID
            assert b"min_agree" in lib.smvs_last_error()
    # the view entries also check what the `_opts` entries check
    for call in calls[:2]:
        for winner in (2, -1):
            assert call(_view_options(winner=winner)) == INVALID
            assert b"winner" in lib.smvs_last_error()
        for merge in (0, 1):
            assert call(_view_options(p2_mode=3, merge=merge)) == INVALID
            assert b"mode" in lib.smvs_last_error()
            assert call(_view_options(merge=merge), num_steps=132) == INVALID
            assert b"multiple of 8 in [136, 256]" in lib.smvs_last_error()
    # three neighbours through the entry of the reference's merge: as before
    w, h = 24, 16
    main = np.full((h, w), 90, np.uint8)
    arr = _neighbors(3, main)
    depth = np.zeros((h, w), np.float32)
    opts = SgmOptions(0, 0)
    rc = lib.smvs_sgm_depth_for_view_opts(
        0, main.ctypes.data_as(C.POINTER(C.c_uint8)), w, h, arr, 3, 16, C.c_uint16(6),
        C.c_uint16(96), C.byref(opts), depth.ctypes.data_as(C.POINTER(C.c_float)))
    assert rc == INVALID and b"one or two neighbours" in lib.smvs_last_error()
    assert C.sizeof(SgmNeighbor) > 0


def test_python_fronts_refuse_before_the_device():
    from smvs_amd import _capi, device
    main = np.full((16, 24), 90, np.uint8)
    nb = dict(image=main, M_fwd=np.eye(3), t_fwd=[-6, 0, 0], M_bwd=np.eye(3), t_bwd=[6, 0, 0],
              range_main=[1, 8], range_neighbor=[1, 8])
    with pytest.raises(_capi.SmvsError):
        device.sgm_depth_for_view(main, [nb] * 3, num_steps=16, consensus=True, agree_ratio=1.5)
    with pytest.raises(_capi.SmvsError):
        device.sgm_depth_for_view(main, [nb] * 3, num_steps=16)     # the reference's merge
    with pytest.raises(ValueError):
        device.sgm_depth_for_view(main, [nb] * 2, num_steps=16, want_checked=True)
    with pytest.raises(_capi.SmvsError):
        device.sgm_check_merge(np.ones((2, 16, 24), F),
                               [dict(bwd=np.ones((16, 24), F), M_fwd=np.eye(3), t_fwd=[0, 0, 0])] * 2,
                               agree_ratio=0.5, min_agree=0)


def test_host_and_python_options_default_to_off():
    """4. SGMStereo::Options and ReconSettings hold (2 neighbours, no consensus,
    0.95, 2) when default-constructed, the Python fronts default to the same,
    and three neighbours without the consensus are an error, not a truncation."""
    from smvs_amd import _capi, device, host, synth
    hlib = host.load()
    for name in ("smvs_host_sgm_depth_merge", "smvs_host_reconstruct_scene_merge",
                 "smvs_host_sgm_merge_defaults"):
        assert hasattr(hlib, name), name
    ints = (C.c_int * 8)(*([7] * 8))
    ratios = (C.c_float * 2)(7.0, 7.0)
    assert hlib.smvs_host_sgm_merge_defaults(ints, ratios) == 0
    assert list(ints) == [2, 0, 2, 0, 2, 0, 2, 0]
    assert list(ratios) == [F(0.95), F(0.95)]
    assert hlib.smvs_host_sgm_merge_defaults(None, None) != 0
    want = {device.sgm_depth_for_view: dict(consensus=False, agree_ratio=0.95, min_agree=2,
                                            want_checked=False),
            device.sgm_check_merge: dict(agree_ratio=0.95, min_agree=2),
            host.sgm_depth: dict(neighbors=2, consensus=False, agree_ratio=0.95, min_agree=2),
            host.reconstruct_scene: dict(sgm_neighbors=2, sgm_consensus=False,
                                         sgm_agree_ratio=0.95, sgm_min_agree=2)}
    for fn, defaults in want.items():
        for key, value in defaults.items():
            got = inspect.signature(fn).parameters[key].default
            assert got == value and type(got) is type(value), (fn, key)
    assert [f[0] for f in device.SgmViewOptions._fields_] == [
        "p2_mode", "winner", "merge", "min_agree", "agree_ratio"]
    assert C.sizeof(device.SgmViewOptions) == 20
    # more than two neighbours without the consensus: an error before any image
    # is looked at, never the first two
    inputs = synth.pipeline_inputs("plane", 48, 32, 3, n_features=50)
    with pytest.raises(_capi.SmvsError) as e:
        host.sgm_depth(inputs, 1, neighbors=3)
    assert "consensus" in str(e.value)
    # the scene entry checks its arguments first, then reaches the scene
    st = host.ReconSettings(b"undistorted", 1.0, 2, 0, 1, 0, 0, 0, 0.0, 0.0, 1, 6, 3, 0, 1, 2,
                            -1, 1700000)
    n = C.c_int(0)
    hlib.smvs_host_last_error.restype = C.c_char_p

    def scene(neighbors, consensus, ratio, min_agree):
        return hlib.smvs_host_reconstruct_scene_merge(
            b"/nonexistent", C.byref(st), C.c_uint(0), C.c_int(128), C.c_int(0),
            C.c_int(neighbors), C.c_int(consensus), C.c_float(ratio), C.c_int(min_agree), None, 0,
            None, 0, C.byref(n), None, None, None)
    for args in ((3, 0, 0.95, 2), (0, 1, 0.95, 2), (17, 1, 0.95, 2)):
        assert scene(*args) != 0 and b"sgm_neighbors" in hlib.smvs_host_last_error()
    for args in ((4, 1, 1.5, 2), (4, 1, float("nan"), 2), (4, 1, 0.95, 0)):
        assert scene(*args) != 0 and b"sgm_agree_ratio" in hlib.smvs_host_last_error()
    assert scene(4, 1, 0.95, 2) != 0
    assert b"sgm_" not in hlib.smvs_host_last_error()
