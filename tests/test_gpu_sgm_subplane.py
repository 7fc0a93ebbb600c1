"""GPU parity of the sub-plane winner of the SGM front end (DESIGN.md section
3.6, "sub-plane depth"; SMVS_SGM_WINNER_SUBPLANE of include/smvs_hip.h): the
three sub-plane WTA kernels against the numpy restatement
tests/sgm_subplane_ref.py on the oracle's volumes (the adaptive restatement's in
that mode), a view's front end against the composition of the same pieces, and
the optimizer started from the refined map.  The definition fixes every float
operation: every comparison of a depth map is array_equal."""
import ctypes as C

import numpy as np
import pytest

import sgm_adaptive_ref as adaptive_ref  # tests/sgm_adaptive_ref.py
import sgm_subplane_ref as ref           # tests/sgm_subplane_ref.py
from parity_units import assert_same_units  # tests/parity_units.py

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
    return ref.scene_pair()


_COST = {}


def _want(oracle, pair, D, lo, hi, adaptive):
    """cost, S, winners of the oracle (the adaptive restatement's S in that
    mode) and the restatement's sub-plane map; the cost volume of a sweep is
    computed once for both modes."""
    main, nbr, M, t = pair
    key = (D, lo, hi)
    if key not in _COST:
        depths = oracle.sgm_depths(lo, hi, D)
        cost = oracle.sgm_cost_volume(main, nbr, M, t, depths)
        cost.setflags(write=False)
        _COST[key] = (depths, cost)
    depths, cost = _COST[key]
    if adaptive:
        sgm = adaptive_ref.aggregate(cost, main, 6, 96, literal=False)
    else:
        sgm = oracle.sgm_aggregate(cost, 6, 96)
    plane_depth, argmin = oracle.sgm_depth_from_volume(sgm, main, depths)
    return dict(cost=cost, sgm=sgm, argmin=argmin, plane_depth=plane_depth,
                depth=ref.subplane_depth(sgm, argmin, main, lo, hi))


def _run_mode(pair, lo, hi, D, adaptive, want_volumes):
    """smvs_sgm_run_mode itself (device.sgm_run goes through the _opts entry)"""
    from smvs_amd import _capi
    lib = _capi.load()
    main, nbr, M, t = pair
    main = np.ascontiguousarray(main, np.uint8)
    nbr = np.ascontiguousarray(nbr, np.uint8)
    M = np.ascontiguousarray(M, F).reshape(9)
    t = np.ascontiguousarray(t, F).reshape(3)
    h, w = main.shape
    nh, nw = nbr.shape
    u8, fp = C.POINTER(C.c_uint8), C.POINTER(C.c_float)
    u16, i32 = C.POINTER(C.c_uint16), C.POINTER(C.c_int32)
    depth = np.zeros((h, w), F)
    argmin = np.zeros((h, w), np.int32)
    cost = np.zeros((h, w, D), np.uint16) if want_volumes else None
    sgm = np.zeros((h, w, D), np.uint16) if want_volumes else None
    rc = lib.smvs_sgm_run_mode(0, main.ctypes.data_as(u8), w, h, nbr.ctypes.data_as(u8), nw, nh,
                               M.ctypes.data_as(fp), t.ctypes.data_as(fp), C.c_float(lo),
                               C.c_float(hi), D, C.c_uint16(6), C.c_uint16(96),
                               C.c_int(1 if adaptive else 0), depth.ctypes.data_as(fp),
                               argmin.ctypes.data_as(i32),
                               cost.ctypes.data_as(u16) if want_volumes else None,
                               sgm.ctypes.data_as(u16) if want_volumes else None)
    assert rc == 0, lib.smvs_last_error()
    return dict(depth=depth, argmin=argmin, cost=cost, sgm=sgm)


RUNS = [(128, 3, 12, False), (128, 1, 12, False), (64, 1, 12, False), (33, 1, 12, False),
        (256, 1, 12, False), (200, 1, 12, False), (128, 3, 12, True), (256, 1, 12, True)]


@pytest.mark.parametrize("D,lo,hi,adaptive", RUNS, ids=[
    "%d-%d-%d-%s" % (D, lo, hi, "adaptive" if a else "constant") for D, lo, hi, a in RUNS])
def test_run_matches_the_restatement(hip, oracle, pair, D, lo, hi, adaptive):
    """6. smvs_sgm_run_opts with winner = 1, with every volume and with the
    depth alone (the fused kernels form S in registers only then): cost, sgm,
    argmin are the oracle's (the adaptive restatement's), depth is the
    restatement's on that volume.  With winner = 0 the bytes are
    smvs_sgm_run_mode's.

    Counted on the CPU over the oracle's valid pixels (constant mode):
    (128, 3, 12): 6106 valid, off != 0 at 5854, winner i % 4 == 0 at 1141,
    i % 4 == 3 at 1028, i % 16 == 0 at 215, i % 16 == 15 at 243, i % 64 == 63 at
    54, i >= 64 at 3578, the last plane at 53; (256, 1, 12): i % 64 == 0 at
    266, i % 64 == 63 at 231, i >= 128 at 184; (33, 1, 12): 5156 valid.
    den == 0 under a valid winner below the last plane: none."""
    main, nbr, M, t = pair
    want = _want(oracle, pair, D, lo, hi, adaptive)
    i = want["argmin"]
    v = want["plane_depth"] > 0
    off, den, _ = ref.winner_offsets(want["sgm"], i)
    count = {
        "valid": int(v.sum()), "off != 0": int((off[v] != 0).sum()),
        "i % 4 == 0": int((i[v] % 4 == 0).sum()), "i % 4 == 3": int((i[v] % 4 == 3).sum()),
        "i % 16 == 0": int((i[v] % 16 == 0).sum()), "i % 16 == 15": int((i[v] % 16 == 15).sum()),
        "i % 64 == 0": int((i[v] % 64 == 0).sum()), "i % 64 == 63": int((i[v] % 64 == 63).sum()),
        "i >= 64": int((i[v] >= 64).sum()), "i >= 128": int((i[v] >= 128).sum()),
        "last plane": int((i[v] == D - 1).sum()),
        "den == 0 below the last plane": int((den[v & (i < D - 1)] == 0).sum())}
    print("%s: %s" % ((D, lo, hi, adaptive), count))
    # the comparison does not pass emptily
    assert count["valid"] >= 1 and count["off != 0"] >= 1
    if (D, lo, hi) == (128, 3, 12):
        for key in ("i % 4 == 0", "i % 4 == 3", "i % 16 == 0", "i % 16 == 15", "i % 64 == 63",
                    "i >= 64", "last plane"):
            assert count[key] >= 1, key
    if (D, lo, hi) == (256, 1, 12):
        for key in ("i % 64 == 0", "i % 64 == 63", "i >= 128"):
            assert count[key] >= 1, key
    assert not np.array_equal(want["depth"], want["plane_depth"])

    full = hip.sgm_run(main, nbr, M, t, lo, hi, D, 6, 96, want_volumes=True,
                       adaptive_p2=adaptive, subplane=True)
    assert np.array_equal(full["cost"], want["cost"])
    assert np.array_equal(full["sgm"], want["sgm"])
    assert np.array_equal(full["argmin"], want["argmin"])
    assert np.array_equal(full["depth"], want["depth"])
    lean = hip.sgm_run(main, nbr, M, t, lo, hi, D, 6, 96, adaptive_p2=adaptive, subplane=True)
    assert np.array_equal(lean["argmin"], want["argmin"])
    assert np.array_equal(lean["depth"], want["depth"])
    # winner = 0: the bytes of the entry without options
    for volumes in (True, False):
        a = hip.sgm_run(main, nbr, M, t, lo, hi, D, 6, 96, want_volumes=volumes,
                        adaptive_p2=adaptive)
        b = _run_mode(pair, lo, hi, D, adaptive, volumes)
        assert np.array_equal(b["depth"], want["plane_depth"])
        for key in ("depth", "argmin") + (("cost", "sgm") if volumes else ()):
            assert a[key].tobytes() == b[key].tobytes(), key


# ------------------------------------------------------------ a view's front end
@pytest.fixture(scope="module")
def scene_inputs():
    from smvs_amd import synth
    return synth.pipeline_inputs("sphere", 384, 256, 3, flen=1.2)


def _front_end_inputs(inputs):
    """The SGM-scale images, reprojections and depth ranges of the main view and
    its first two neighbours, as smvs_sgm_depth_for_view wants them
    (tests/test_gpu_sgm_wide.py)."""
    from smvs_amd import host
    imgs = [host.sgm_image(inputs, k, 1) for k in range(3)]
    small = dict(inputs, images=imgs)
    nbs = []
    for k in (1, 2):
        Mf, tf = host.view_reprojection(small, 0, k)
        Mb, tb = host.view_reprojection(small, k, 0)
        nbs.append(dict(image=imgs[k], M_fwd=Mf, t_fwd=tf, M_bwd=Mb, t_bwd=tb,
                        range_main=host.depth_range(inputs, 0),
                        range_neighbor=host.depth_range(inputs, k)))
    return imgs[0], nbs


def _merge(first, second):
    """app/smvsrecon.cc:366-377"""
    return np.where(second == 0, first, np.where(first == 0, second,
                    (first + second) * F(0.5))).astype(F)


def _reference_front_end(oracle, main, nbs, D, adaptive):
    """4 runs (oracle cost volume, oracle or adaptive-restatement aggregation,
    oracle winners), each as the plane's depth and refined by the restatement;
    for both oracle.sgm_lr_check and the reference's merge.
    -> {subplane: (merged map, the two checked maps)}"""
    def run(a, b, M, t, rng):
        depths = oracle.sgm_depths(rng[0], rng[1], D)
        cost = oracle.sgm_cost_volume(a, b, M, t, depths)
        sgm = (adaptive_ref.aggregate(cost, a, 6, 96, literal=False) if adaptive
               else oracle.sgm_aggregate(cost, 6, 96))
        plane, argmin = oracle.sgm_depth_from_volume(sgm, a, depths)
        return {False: plane, True: ref.subplane_depth(sgm, argmin, a, rng[0], rng[1])}
    maps = {False: [], True: []}
    for nb in nbs:
        fwd = run(main, nb["image"], nb["M_fwd"], nb["t_fwd"], nb["range_main"])
        bwd = run(nb["image"], main, nb["M_bwd"], nb["t_bwd"], nb["range_neighbor"])
        for sub in (False, True):
            maps[sub].append(oracle.sgm_lr_check(fwd[sub], bwd[sub], nb["M_fwd"], nb["t_fwd"]))
    return {sub: (_merge(*maps[sub]), maps[sub]) for sub in (False, True)}


_FRONT = {}


def _front(oracle, scene_inputs, D, adaptive, subplane):
    """The reference front end of the scene, computed once per (D, mode)."""
    key = (D, adaptive)
    if key not in _FRONT:
        main, nbs = _front_end_inputs(scene_inputs)
        _FRONT[key] = _reference_front_end(oracle, main, nbs, D, adaptive)
        for merged, _ in _FRONT[key].values():
            merged.setflags(write=False)
    return _FRONT[key][subplane]


@pytest.mark.parametrize("D,adaptive", [(128, False), (256, False), (128, True)],
                         ids=["128", "256", "128-adaptive"])
def test_view_front_end_matches_the_composition(hip, oracle, scene_inputs, D, adaptive):
    """7. host.sgm_depth(subplane=True) and device.sgm_depth_for_view on
    SGM-scale and on raw images == forward and backward runs refined by the
    restatement, the oracle's L/R check, the reference's merge.  The map
    differs from the integer one on more than half of its valid pixels; the
    zero sets differ only where a run's L/R check decides otherwise."""
    from smvs_amd import host
    want, sub_maps = _front(oracle, scene_inputs, D, adaptive, True)
    plane, plane_maps = _front(oracle, scene_inputs, D, adaptive, False)
    valid = want > 0
    assert valid.mean() > 0.5
    assert ((want != plane) & valid).sum() > 0.5 * valid.sum()
    # before the check the zero sets are the same (the validity rule is), so a
    # pixel can only change sides where the check of a run decides otherwise
    flips = np.zeros(want.shape, bool)
    for a, b in zip(sub_maps, plane_maps):
        flips |= (a != 0) != (b != 0)
    zero_diff = (want == 0) != (plane == 0)
    print("D %d adaptive %s: L/R decisions that differ at %d pixels, zero sets at %d of %d"
          % (D, adaptive, int(flips.sum()), int(zero_diff.sum()), want.size))
    assert not np.any(zero_diff & ~flips)

    if not adaptive:
        # the integer composition is the oracle's own front end
        assert np.array_equal(plane, oracle.sgm_depth_for_view(scene_inputs, sgm_scale=1,
                                                               num_steps=D))
    got = host.sgm_depth(scene_inputs, 1, adaptive_penalty2=adaptive, num_steps=D, subplane=True)
    assert np.array_equal(got, want)
    main, nbs = _front_end_inputs(scene_inputs)
    assert np.array_equal(hip.sgm_depth_for_view(main, nbs, num_steps=D, adaptive_p2=adaptive,
                                                 subplane=True), want)
    raw = [dict(nb, image=scene_inputs["images"][k]) for nb, k in zip(nbs, (1, 2))]
    assert np.array_equal(hip.sgm_depth_for_view(scene_inputs["images"][0], raw, num_steps=D,
                                                 adaptive_p2=adaptive, halvings=1,
                                                 subplane=True), want)
    # off: the integer map, as before
    assert np.array_equal(host.sgm_depth(scene_inputs, 1, adaptive_penalty2=adaptive,
                                         num_steps=D), plane)


def _rel(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b) / max(np.linalg.norm(b), 1e-300))


def test_optimize_from_the_subplane_map_matches_oracle(hip, oracle, scene_inputs):
    """8. DepthOptimizer::optimize started from the sub-plane map: C++ host +
    HIP against the oracle's optimiser started from the reference map of test
    7 (through write_depth_to_view / get_sgm_depth, whose host mirror the
    integer maps of tests/test_gpu_parity.py pin to the oracle's bit for bit).
    The units and bounds of the SGM-initialised case of tests/test_gpu_front.py:
    batch log in the bench metric's units (tests/parity_units.py, no drift
    allowance), the valid pixels identical, depth within 1e-4 relative L2."""
    from smvs_amd import host
    want_map = _front(oracle, scene_inputs, 128, False, True)[0]
    sgm = host.sgm_depth(scene_inputs, sgm_scale=1, subplane=True)
    assert np.array_equal(sgm, want_map)
    got = host.optimize(scene_inputs, regularization=0.01, num_iterations=5, min_scale=2,
                        sgm_depth=sgm)
    want = oracle.optimize(scene_inputs, regularization=0.01, num_iterations=5, min_scale=2,
                           sgm_depth=got["sgm_roundtrip"])
    assert_same_units(got["log"], want["log"], 384, 256, "sgm_subplane_384x256")
    assert np.array_equal(got["depth"] > 0, want["depth"] > 0)
    assert (want["depth"] > 0).mean() > 0.5
    print("depth rel L2 %.3e" % _rel(got["depth"], want["depth"]))
    assert _rel(got["depth"], want["depth"]) <= 1e-4
