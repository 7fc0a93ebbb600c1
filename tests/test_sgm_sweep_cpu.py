"""CPU checks of the multi-neighbour plane sweep of the SGM front end (DESIGN.md
section 3.6, "plane sweep"; include/smvs_hip.h, "Multi-neighbour plane sweep"):
properties of the numpy restatement tests/sgm_sweep_ref.py, the argument checks
of the three new entries, which need no GPU, the defaults of the host mirror and
the Python fronts, and the branches of the definition on a small scene."""
import ctypes as C
import inspect

import numpy as np
import pytest

import sgm_sweep_compose as compose  # tests/sgm_sweep_compose.py
import sgm_sweep_ref as ref          # tests/sgm_sweep_ref.py

INVALID = -1


def _random_costs(n, shape, seed):
    """bytes over 0 .. 255 with 255 at about a quarter of the positions"""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 256, (n,) + shape).astype(np.uint8)
    c[rng.random((n,) + shape) < 0.25] = 255
    return c


# ------------------------------------------------------------- the restatement
def test_fold_by_hand():
    """A table worked out by hand: columns are cells, rows neighbours."""
    c = np.array([[10, 255, 255, 3, 0, 254],
                  [13, 255, 7, 4, 1, 254],
                  [255, 255, 255, 8, 1, 255],
                  [40, 255, 255, 255, 255, 255]], np.uint8)
    # all costs: (10+13+40)/3 = 21; none; one; (3+4+8)/3 = 5; 2/3 -> 1; 254
    assert list(ref.fold(c, 1, 0)) == [21, 255, 7, 5, 1, 254]
    # at least two costs
    assert list(ref.fold(c, 2, 0)) == [21, 255, 255, 5, 1, 254]
    # the two smallest: 23/2 -> 12 (half up); 7; 7/2 -> 4 (half up); 1/2 -> 1 (half up)
    assert list(ref.fold(c, 1, 2)) == [12, 255, 7, 4, 1, 254]
    assert list(ref.fold(c, 3, 1)) == [10, 255, 255, 3, 0, 255]
    parts = ref.fold_parts(c, 2, 2)
    assert list(parts["m"]) == [3, 0, 1, 3, 3, 2]
    assert list(parts["k_eff"]) == [2, 0, 0, 2, 2, 2]
    assert list(parts["S"]) == [23, 0, 0, 7, 1, 508]


@pytest.mark.parametrize("n", [1, 2, 3, 6, 16])
def test_restatement_properties(n):
    """1. The two identities of the definition -- n = 1 with min_views = 1 gives
    c[0]; j copies of one neighbour give that neighbour's volume for any best_k
    -- the invariance under permuting the neighbours, and, on input sorted along
    the neighbours, the fold monotone (not decreasing) in best_k, with best_k = 0
    standing behind n."""
    shape = (37, 30)
    c = _random_costs(n, shape, 100 + n)
    one = c[0]
    assert np.array_equal(ref.fold(one[None], 1, 0), one)
    assert np.array_equal(ref.fold(one[None], 1, 5), one)
    for best_k in (0, 1, (n + 1) // 2, n, 16):
        for min_views in sorted({1, n}):
            assert np.array_equal(ref.fold(np.stack([one] * n), min_views, best_k), one), best_k
    perm = np.random.default_rng(7).permutation(n)
    for min_views in sorted({1, min(2, n), n}):
        for best_k in (0, 1, (n + 1) // 2, n):
            assert np.array_equal(ref.fold(c[perm], min_views, best_k),
                                  ref.fold(c, min_views, best_k))
    ordered = np.sort(c, axis=0)
    folds = [ref.fold(ordered, 1, k).astype(int) for k in list(range(1, n + 1)) + [0]]
    for a, b in zip(folds, folds[1:]):
        assert np.all(a <= b)
    assert np.array_equal(folds[-1], folds[-2])     # best_k = n looks at all, as 0 does
    # the support counts what it says
    argmin = np.random.default_rng(8).integers(0, 30, (5, 37))
    vols = _random_costs(n, (5, 37, 30), 200 + n)
    sup = ref.support(vols, argmin, 100)
    y, x = 3, 11
    assert sup[y, x] == sum(int(vols[j, y, x, argmin[y, x]]) <= 100 for j in range(n))
    assert sup.dtype == np.uint8 and sup.max() <= n


# ------------------------------------------------------------------ the entries
def _hip_lib():
    from smvs_amd import _capi
    lib = _capi.load()
    lib.smvs_last_error.restype = C.c_char_p
    return lib


W, H = 24, 16
GOOD = dict(p2_mode=0, winner=0, min_views=1, best_k=0, support_cost=20, min_support=0)


def _options(**kw):
    from smvs_amd.device import SgmSweepOptions
    o = dict(GOOD, **kw)
    return SgmSweepOptions(o["p2_mode"], o["winner"], o["min_views"], o["best_k"],
                           o["support_cost"], o["min_support"])


def _sweep(lib, opts, raw, n=3, rng=(1.0, 8.0), num_steps=16, p1=6, p2=96):
    from smvs_amd import device
    main = np.full((H, W, 3) if raw else (H, W), 90, np.uint8)
    nb = dict(image=main, M_fwd=np.eye(3), t_fwd=[-6, 0, 0], M_bwd=np.eye(3), t_bwd=[6, 0, 0],
              range_main=[1, 8], range_neighbor=[1, 8])
    keep = []
    arr = device._sgm_neighbors([nb] * max(n, 1), keep)
    u8p, fp = C.POINTER(C.c_uint8), C.POINTER(C.c_float)
    depth = np.zeros((H, W), np.float32)
    r = (C.c_float * 2)(*rng) if rng is not None else None
    o = C.byref(opts) if opts is not None else None
    if raw:
        nch = (C.c_int * max(n, 1))(*([3] * max(n, 1)))
        return lib.smvs_sgm_sweep_for_view_raw(0, main.ctypes.data_as(u8p), W, H, 3, arr, nch, n, 0,
                                               r, num_steps, C.c_uint16(p1), C.c_uint16(p2), o,
                                               depth.ctypes.data_as(fp), None)
    return lib.smvs_sgm_sweep_for_view(0, main.ctypes.data_as(u8p), W, H, arr, n, r, num_steps,
                                       C.c_uint16(p1), C.c_uint16(p2), o,
                                       depth.ctypes.data_as(fp), None, None, None, None)


def _fold(lib, n=3, min_views=1, best_k=0, length=64):
    costs = np.zeros((max(n, 1), max(length, 1)), np.uint8)
    out = np.zeros(max(length, 1), np.uint8)
    u8p = C.POINTER(C.c_uint8)
    return lib.smvs_sgm_fold_costs(0, costs.ctypes.data_as(u8p), n, C.c_size_t(length), min_views,
                                   best_k, out.ctypes.data_as(u8p))


def test_sweep_entries_exist_and_refuse_bad_arguments_without_a_gpu():
    """2. smvs_sgm_sweep_for_view, ..._raw and smvs_sgm_fold_costs are exported
    and answer SMVS_ERR_INVALID with a message that names the argument -- before
    any device call, so also on a machine without a GPU -- to every argument
    outside the accepted set of include/smvs_hip.h."""
    from smvs_amd import _capi
    lib = _hip_lib()
    for name in ("smvs_sgm_sweep_for_view", "smvs_sgm_sweep_for_view_raw", "smvs_sgm_fold_costs"):
        assert name in _capi.declared_symbols() and hasattr(lib, name), name

    def refused(rc, word):
        assert rc == INVALID
        assert word in lib.smvs_last_error(), (word, lib.smvs_last_error())

    for raw in (False, True):
        def call(opts, **kw):
            return _sweep(lib, opts, raw, **kw)
        refused(call(None), b"options")
        for n in (0, 17, -1):
            refused(call(_options(), n=n), b"n_neighbors")
        for min_views in (0, 4, -1):
            refused(call(_options(min_views=min_views)), b"min_views")
        for best_k in (-1, 17):
            refused(call(_options(best_k=best_k)), b"best_k")
        for support_cost in (-1, 255, 1000):
            refused(call(_options(support_cost=support_cost)), b"support_cost")
        for min_support in (-1, 4):
            refused(call(_options(min_support=min_support)), b"min_support")
        for rng in ((0.0, 8.0), (-1.0, 8.0), (3.0, 3.0), (8.0, 1.0), (float("nan"), 8.0),
                    (1.0, float("nan"))):
            refused(call(_options(), rng=rng), b"depth range")
        refused(call(_options(), rng=None), b"range")
        for winner in (2, -1):
            refused(call(_options(winner=winner)), b"winner")
        refused(call(_options(p2_mode=3)), b"mode")
        for num_steps in (1, 132, 264):
            refused(call(_options(), num_steps=num_steps), b"multiple of 8 in [136, 256]")
        refused(call(_options(), p1=100, p2=50), b"penalty2")
        refused(call(_options(), p2=9000), b"penalty2")
        # the accepted corners pass the checks (and then need a device or run)
        for good in (_options(min_views=3, best_k=16, support_cost=254, min_support=3),
                     _options(best_k=0, support_cost=0)):
            rc = call(good)
            assert rc == 0 or b"must be" not in lib.smvs_last_error()
    for n in (0, 17, -1):
        refused(_fold(lib, n=n), b"n_neighbors")
    for min_views in (0, 4):
        refused(_fold(lib, min_views=min_views), b"min_views")
    for best_k in (-1, 17):
        refused(_fold(lib, best_k=best_k), b"best_k")
    refused(_fold(lib, length=0), b"len")
    u8p = C.POINTER(C.c_uint8)
    out = np.zeros(4, np.uint8)
    refused(lib.smvs_sgm_fold_costs(0, None, 1, C.c_size_t(4), 1, 0, out.ctypes.data_as(u8p)), b"null")
    refused(lib.smvs_sgm_fold_costs(0, out.ctypes.data_as(u8p), 1, C.c_size_t(4), 1, 0, None), b"null")


def test_host_and_python_options_default_to_off():
    """3. SGMStereo::Options and ReconSettings hold (no sweep, -1, -1, 20, -1) when
    default-constructed (-1: the default at n neighbours), the Python fronts
    default to the same, the default at n neighbours is (min(2, n), (n + 1) / 2,
    20, min(2, n)), and the sweep together with the consensus is an error in the
    host mirror, as is a value outside the accepted set in the scene entry."""
    from smvs_amd import _capi, device, host, synth
    hlib = host.load()
    hlib.smvs_host_last_error.restype = C.c_char_p
    for name in ("smvs_host_sgm_depth_sweep", "smvs_host_reconstruct_scene_sweep",
                 "smvs_host_sgm_sweep_defaults"):
        assert hasattr(hlib, name), name
    ints = (C.c_int * 10)(*([7] * 10))
    assert hlib.smvs_host_sgm_sweep_defaults(ints) == 0
    assert list(ints) == [0, -1, -1, 20, -1] * 2
    assert hlib.smvs_host_sgm_sweep_defaults(None) != 0
    want = {device.sgm_sweep_for_view: dict(min_views=None, best_k=None, support_cost=20,
                                            min_support=None, adaptive_p2=False, subplane=False),
            device.sgm_fold_costs: dict(min_views=1, best_k=0),
            host.sgm_depth: dict(sweep=False, sweep_min_views=-1, sweep_best_k=-1,
                                 sweep_support_cost=20, sweep_min_support=-1),
            host.reconstruct_scene: dict(sgm_sweep=False, sgm_sweep_min_views=-1,
                                         sgm_sweep_best_k=-1, sgm_sweep_support_cost=20,
                                         sgm_sweep_min_support=-1)}
    for fn, defaults in want.items():
        for key, value in defaults.items():
            got = inspect.signature(fn).parameters[key].default
            assert got == value and type(got) is type(value), (fn, key)
    assert [device.sgm_sweep_defaults(n) for n in (1, 2, 3, 4, 6, 16)] == [
        (1, 1, 20, 1), (2, 1, 20, 2), (2, 2, 20, 2), (2, 2, 20, 2), (2, 3, 20, 2), (2, 8, 20, 2)]
    assert [f[0] for f in device.SgmSweepOptions._fields_] == [
        "p2_mode", "winner", "min_views", "best_k", "support_cost", "min_support"]
    assert C.sizeof(device.SgmSweepOptions) == 24 and C.sizeof(host.SgmSweep) == 20
    inputs = synth.pipeline_inputs("plane", 48, 32, 3, n_features=50)
    with pytest.raises(_capi.SmvsError) as e:
        host.sgm_depth(inputs, 1, neighbors=3, sweep=True, consensus=True)
    assert "sweep" in str(e.value) and "consensus" in str(e.value)
    with pytest.raises(_capi.SmvsError) as e:
        host.sgm_depth(inputs, 1, neighbors=3)      # neither: the error it was
    assert "consensus" in str(e.value)
    st = host.ReconSettings(b"undistorted", 1.0, 2, 0, 1, 0, 0, 0, 0.0, 0.0, 1, 6, 3, 0, 1, 2,
                            -1, 1700000)
    n = C.c_int(0)

    def scene(neighbors, consensus, sweep):
        sw = host.SgmSweep(*sweep)
        return hlib.smvs_host_reconstruct_scene_sweep(
            b"/nonexistent", C.byref(st), C.c_uint(0), C.c_int(128), C.c_int(0),
            C.c_int(neighbors), C.c_int(consensus), C.c_float(0.95), C.c_int(2), C.byref(sw),
            None, 0, None, 0, C.byref(n), None, None, None)
    assert scene(4, 1, (1, -1, -1, 20, -1)) != 0
    assert b"exclude each other" in hlib.smvs_host_last_error()
    assert scene(4, 0, (0, -1, -1, 20, -1)) != 0 and b"sgm_neighbors" in hlib.smvs_host_last_error()
    assert scene(17, 0, (1, -1, -1, 20, -1)) != 0
    assert b"sgm_neighbors" in hlib.smvs_host_last_error()
    for sweep in ((1, 0, -1, 20, -1), (1, -1, 17, 20, -1), (1, -1, -1, 255, -1),
                  (1, -1, -1, 20, 17), (1, -2, -1, 20, -1)):
        assert scene(4, 0, sweep) != 0 and b"sgm_sweep_" in hlib.smvs_host_last_error(), sweep
    # accepted: the call gets as far as the scene, which is not there
    assert scene(6, 0, (1, -1, -1, 20, -1)) != 0
    assert b"sgm_" not in hlib.smvs_host_last_error()


def test_python_fronts_refuse_before_the_device():
    from smvs_amd import _capi, device
    main = np.full((16, 24), 90, np.uint8)
    nb = dict(image=main, M_fwd=np.eye(3), t_fwd=[-6, 0, 0])
    with pytest.raises(_capi.SmvsError):
        device.sgm_sweep_for_view(main, [nb] * 3, (1, 8), num_steps=16, min_views=4)
    with pytest.raises(_capi.SmvsError):
        device.sgm_sweep_for_view(main, [nb] * 3, (8, 1), num_steps=16)
    with pytest.raises(_capi.SmvsError):
        device.sgm_sweep_for_view(main, [], (1, 8), num_steps=16)
    with pytest.raises(ValueError):
        device.sgm_sweep_for_view(main, [nb], (1, 8), num_steps=16, halvings=0, want_volumes=True)
    with pytest.raises(_capi.SmvsError):
        device.sgm_fold_costs(np.zeros((3, 40), np.uint8), min_views=1, best_k=17)
    with pytest.raises(ValueError):
        device.sgm_fold_costs(np.zeros(40, np.uint8))


# ------------------------------------------------- the branches, on a small scene
def test_every_branch_of_the_definition_occurs_on_the_small_sphere(oracle):
    """4. The composition (tests/sgm_sweep_compose.py) on synth.pipeline_inputs(
    "sphere", 96, 64, 6, flen=1.2) at full resolution, 32 planes over 0.8 x min
    to 1.2 x max of the true depth, (min_views, best_k) = (2, 3), support
    (cost <= 10, at least 2): every branch of the definition occurs -- a cell
    without any cost, one with fewer costs than min_views, one with more costs
    than are averaged, a mean rounded up, one rounded down and an exact one, a
    folded byte that no neighbour has, a pixel the support test rejects and one
    it accepts.  The fold of six neighbours also puts more winners within one
    plane of the truth than a single neighbour's volume does."""
    from smvs_amd import synth
    inputs = synth.pipeline_inputs("sphere", 96, 64, 6, flen=1.2)
    main, nbs, _ = compose.front_end_inputs(inputs, 6, halvings=0)
    truth = inputs["truth"]
    assert main.shape == (64, 96) == truth.shape
    rng = (0.8 * float(truth[truth > 0].min()), 1.2 * float(truth.max()))
    D = 32
    got = compose.sweep(oracle, main, nbs, rng, D, min_views=2, best_k=3, support_cost=10,
                        min_support=2)
    vols = got["vols"]
    parts = ref.fold_parts(vols, 2, 3)
    assert np.array_equal(parts["C"], got["cost"])
    m, k_eff, S = parts["m"], parts["k_eff"], parts["S"]
    folded = k_eff > 0
    rem = np.where(folded, (2 * S + k_eff) % np.maximum(2 * k_eff, 1), -1)
    counts = dict(
        no_cost=int((m == 0).sum()),
        below_min_views=int(((m > 0) & (m < 2)).sum()),
        fewer_than_all=int((folded & (k_eff < m)).sum()),
        # (2 S + k) mod 2 k: k is the exact mean, below k it was rounded up, above down
        rounded_up=int((folded & (rem >= 0) & (rem < k_eff)).sum()),
        rounded_down=int((folded & (rem > k_eff)).sum()),
        exact=int((folded & (rem == k_eff)).sum()),
        no_neighbours_byte=int((folded & np.all(vols != got["cost"][None], axis=0)).sum()),
        support_rejects=int(((got["unchecked"] != 0) & (got["depth"] == 0)).sum()),
        support_accepts=int((got["depth"] != 0).sum()))
    print(counts)
    for key, value in counts.items():
        assert value >= 1, key
    assert counts["rounded_up"] + counts["rounded_down"] + counts["exact"] == int(folded.sum())

    # the planes' depths and the truth's plane; a winner within one plane of it
    depths = oracle.sgm_depths(rng[0], rng[1], D)
    true_plane = np.abs(1.0 / depths[None, None, :] - 1.0 / truth[:, :, None]).argmin(axis=2)

    def share(depth, argmin):
        valid = (depth != 0) & (truth > 0)
        return float((np.abs(argmin - true_plane)[valid] <= 1).mean()), float(valid.mean())
    one = compose.sweep(oracle, main, nbs[:1], rng, D, vols=vols[:1])
    s1, c1 = share(one["unchecked"], one["argmin"])
    s6, c6 = share(got["unchecked"], got["argmin"])
    s6s, c6s = share(got["depth"], got["argmin"])
    print("within one plane: one neighbour %.3f (coverage %.3f), fold of six %.3f (%.3f), "
          "with the support test %.3f (%.3f)" % (s1, c1, s6, c6, s6s, c6s))
    assert s6 > s1
