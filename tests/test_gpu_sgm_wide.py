"""GPU parity of the SGM plane counts above 128 ("plane
counts": the multiples of 8 from 136 to 256, sgm_paths_wide_kernel of
sgm_paths.hip and sgm_sum_wta_wide_kernel of sgm_wta.hip) against the oracle's pieces -- cost volume, the
literal aggregation loop, the WTA -- and, for the adaptive-penalty mode, the
serial restatement tests/sgm_adaptive_reference.cc in its literal form.  The
path is integer: every comparison is array_equal."""
import ctypes as C
import os

import numpy as np
import pytest

import sgm_adaptive_ref as ref  # tests/sgm_adaptive_ref.py

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import smvs_amd
    if smvs_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on a GPU")
    return smvs_amd


def _pair(w, h):
    """Random texture, the neighbour shifted by six pixels; the reprojection of
    tests/test_gpu_sgm_adaptive.py::_crop_pair."""
    base = np.random.default_rng(0).integers(30, 220, (h, w + 40)).astype(np.uint8)
    main = np.ascontiguousarray(base[:, 20:20 + w])
    nbr = np.ascontiguousarray(base[:, 14:14 + w])
    M = np.array([1.001, 0.002, 0.1, -0.001, 0.999, 0.2, 1e-6, -2e-6, 1.0], np.float32)
    t = np.array([-6.0, 0.3, 0.01], np.float32)
    return main, nbr, M, t


_COST = {}


def _oracle_cost(oracle, w, h, D):
    """The oracle's cost volume of a case, computed once for both modes."""
    key = (w, h, D)
    if key not in _COST:
        main, nbr, M, t = _pair(w, h)
        depths = oracle.sgm_depths(1.0, 12.0, D)
        cost = oracle.sgm_cost_volume(main, nbr, M, t, depths)
        cost.setflags(write=False)
        _COST[key] = (depths, cost)
    return _COST[key]


def _want(oracle, w, h, D, p1, p2, adaptive):
    main = _pair(w, h)[0]
    depths, cost = _oracle_cost(oracle, w, h, D)
    if adaptive:
        sgm = ref.aggregate(cost, main, p1, p2, literal=True)
    else:
        sgm = oracle.sgm_aggregate(cost, p1, p2, literal=True)
    depth, argmin = oracle.sgm_depth_from_volume(sgm, main, depths)
    return dict(cost=cost, sgm=sgm, depth=depth, argmin=argmin)


BOTH = (False, True)
CASES = [
    # (w, h, D, P1, P2), modes
    ((64, 40, 256, 6, 96), BOTH),      # every lane busy, the FULL variant
    ((70, 33, 200, 6, 96), BOTH),      # idle lanes, odd line counts, 8 | D but not 16
    ((64, 40, 136, 6, 96), BOTH),      # the first count above 128: two lanes past the half wave
    ((64, 40, 256, 10, 300), BOTH),    # the u16 volume with atomics at 256
    ((48, 32, 256, 170, 255), BOTH),   # the largest penalties of the byte form
    ((48, 32, 256, 171, 255), (True,)),  # P1 * 3 / 2 = 256: one past the byte form
    ((12, 9, 256, 6, 96), BOTH),       # diagonals shorter than a chunk
    ((11, 9, 136, 6, 96), BOTH),       # the smallest image the entry takes
    ((64, 40, 128, 6, 96), BOTH),      # the existing kernel still serves 128
]
PARAMS = [pytest.param(case, adaptive, id="%dx%dx%d-p%d-%d-%s" % (case + ("adaptive" if adaptive
                                                                       else "constant",)))
          for case, modes in CASES for adaptive in modes]


@pytest.mark.parametrize("case,adaptive", PARAMS)
def test_run_matches_the_literal_loop(hip, oracle, case, adaptive):
    """cost, sgm, argmin, depth of smvs_sgm_run_mode == the oracle's cost volume,
    the literal aggregation loop and the oracle's WTA; again without the volumes
    (S is then never formed in memory)."""
    w, h, D, p1, p2 = case
    main, nbr, M, t = _pair(w, h)
    want = _want(oracle, w, h, D, p1, p2, adaptive)
    got = hip.sgm_run(main, nbr, M, t, 1.0, 12.0, D, p1, p2, want_volumes=True,
                      adaptive_p2=adaptive)
    high = float((want["argmin"] >= 128).mean())
    print("argmin >= 128 at %.3f of the pixels, max %d" % (high, want["argmin"].max()))
    assert np.array_equal(got["cost"], want["cost"])
    assert np.array_equal(got["sgm"], want["sgm"])
    assert np.array_equal(got["argmin"], want["argmin"])
    assert np.array_equal(got["depth"], want["depth"])
    lean = hip.sgm_run(main, nbr, M, t, 1.0, 12.0, D, p1, p2, adaptive_p2=adaptive)
    assert np.array_equal(lean["depth"], want["depth"])
    assert np.array_equal(lean["argmin"], want["argmin"])
    if case in ((64, 40, 256, 6, 96), (70, 33, 200, 6, 96)):
        # the planes above 128 win somewhere: the cases do not pass emptily
        assert high >= 0.10
    if adaptive and p2 > p1 * 3 // 2:
        # penalty2 has room above its floor: the mode is not the constant one
        other = _want(oracle, w, h, D, p1, p2, False)
        assert not np.array_equal(other["sgm"], want["sgm"])


# ------------------------------------------------------------ a view's front end
@pytest.fixture(scope="module")
def scene_inputs():
    from smvs_amd import synth
    return synth.pipeline_inputs("sphere", 384, 256, 3, flen=1.2)


def _front_end_inputs(inputs):
    """The SGM-scale images, reprojections and depth ranges of the main view and
    its first two neighbours, as smvs_sgm_depth_for_view wants them."""
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


def _adaptive_front_end(oracle, main, nbs, D, p1=6, p2=96):
    """The front end with the adaptive restatement (closed form, which
    tests/test_sgm_wide_cpu.py shows equal to the literal loop) for the
    aggregation and the oracle for everything else."""
    def run(a, b, M, t, rng):
        depths = oracle.sgm_depths(rng[0], rng[1], D)
        cost = oracle.sgm_cost_volume(a, b, M, t, depths)
        sgm = ref.aggregate(cost, a, p1, p2, literal=False)
        return oracle.sgm_depth_from_volume(sgm, a, depths)[0]
    maps = []
    for nb in nbs:
        fwd = run(main, nb["image"], nb["M_fwd"], nb["t_fwd"], nb["range_main"])
        bwd = run(nb["image"], main, nb["M_bwd"], nb["t_bwd"], nb["range_neighbor"])
        maps.append(oracle.sgm_lr_check(fwd, bwd, nb["M_fwd"], nb["t_fwd"]))
    first, second = maps
    return np.where(second == 0, first, np.where(first == 0, second,
                    (first + second) * np.float32(0.5)))


@pytest.fixture(scope="module")
def view_maps(oracle, scene_inputs):
    """The oracle's front end of the scene at 256 and at 128 planes."""
    m256 = oracle.sgm_depth_for_view(scene_inputs, sgm_scale=1, num_steps=256)
    m128 = oracle.sgm_depth_for_view(scene_inputs, sgm_scale=1, num_steps=128)
    m256.setflags(write=False)
    m128.setflags(write=False)
    return m256, m128


def test_view_front_end_at_256_planes(hip, oracle, scene_inputs, view_maps):
    """host.sgm_depth and device.sgm_depth_for_view (SGM-scale and raw images)
    at 256 planes == the oracle's front end, which differs from its 128-plane
    map"""
    from smvs_amd import host
    want, at128 = view_maps
    assert (want > 0).mean() > 0.5
    assert (want != at128).mean() > 0.5
    assert np.array_equal(host.sgm_depth(scene_inputs, 1, num_steps=256), want)
    assert np.array_equal(host.sgm_depth(scene_inputs, 1), at128)
    main, nbs = _front_end_inputs(scene_inputs)
    assert np.array_equal(hip.sgm_depth_for_view(main, nbs, num_steps=256), want)
    raw = [dict(nb, image=scene_inputs["images"][k]) for nb, k in zip(nbs, (1, 2))]
    assert np.array_equal(hip.sgm_depth_for_view(scene_inputs["images"][0], raw, num_steps=256,
                                                 halvings=1), want)


def test_view_front_end_at_256_planes_adaptive(hip, oracle, scene_inputs, view_maps):
    from smvs_amd import host
    main, nbs = _front_end_inputs(scene_inputs)
    want = _adaptive_front_end(oracle, main, nbs, 256)
    assert (want > 0).mean() > 0.5
    assert not np.array_equal(want, view_maps[0])
    got = host.sgm_depth(scene_inputs, 1, adaptive_penalty2=True, num_steps=256)
    assert np.array_equal(got, want)
    assert np.array_equal(hip.sgm_depth_for_view(main, nbs, num_steps=256, adaptive_p2=True),
                          want)


# --------------------------------------------------------------------- the scene
def _stored(inputs, z):
    """What write_depth_to_view stores for the z-depth map z as "smvs-sgm"
    (MVE's ray-length convention), through the unchanged host mirror."""
    from smvs_amd import host
    host.optimize(inputs, regularization=0.01, num_iterations=1, min_scale=2, sgm_depth=z)
    return host.last_embeddings()["smvs-sgm"]


def _sgm_file(d):
    with open(os.path.join(d, "views", "view_0000.mve", "smvs-sgm.mvei"), "rb") as f:
        return f.read()


def test_reconstruct_scene_passes_the_plane_count_down(hip, oracle, scene_inputs, tmp_path):
    """ReconSettings::sgm_num_steps: the smvs-sgm embedding of the scene run at
    256 planes is the view-level front end for the neighbours ViewSelection
    chose and differs from the 128-plane run's; the default run's embedding is
    the one a run through smvs_host_reconstruct_scene_flags writes."""
    from smvs_amd import host, mve_scene
    inputs = scene_inputs
    scene = dict(views=[dict(id=i, flen=c.flen, rot=c.R, trans=c.t, width=384, height=256)
                        for i, c in enumerate(inputs["cams"])],
                 features=inputs["features"],
                 refs=[list(range(4))] * len(inputs["features"]))
    nb = host.select_neighbors(scene, 0, num_neighbors=3)
    assert len(nb) >= 2
    order = [0] + nb
    sel = dict(inputs, cams=[inputs["cams"][i] for i in order],
               images=[inputs["images"][i] for i in order], view_ids=order)
    want = oracle.sgm_depth_for_view(sel, sgm_scale=1, num_steps=256)
    dirs = {}
    for name in ("wide", "default", "old"):
        dirs[name] = str(tmp_path / name)
        os.makedirs(dirs[name])
        mve_scene.write_scene(dirs[name], inputs)
    done, skipped, _ = host.reconstruct_scene(dirs["wide"], view_ids=[0], num_neighbors=3,
                                              min_neighbors=2, output_scale=2,
                                              sgm_num_steps=256)
    assert done == [0] and skipped == 0
    got = mve_scene.load_mvei(os.path.join(dirs["wide"], "views", "view_0000.mve",
                                           "smvs-sgm.mvei"))
    assert got.shape == (128, 192)
    assert np.array_equal(got, _stored(sel, want))
    done, skipped, _ = host.reconstruct_scene(dirs["default"], view_ids=[0], num_neighbors=3,
                                              min_neighbors=2, output_scale=2)
    assert done == [0] and skipped == 0
    assert _sgm_file(dirs["default"]) != _sgm_file(dirs["wide"])
    # the same settings through the entry that has no plane count
    hlib = host.load()
    st = host.ReconSettings(b"undistorted", 1.0, 2, 0, 1, 0, 0, 0, 0.0, 0.0, 1, 3, 2, 0, 1, 2,
                            -1, 1700000)
    ids = np.array([0], np.int32)
    n = C.c_int(0)
    rc = hlib.smvs_host_reconstruct_scene_flags(
        dirs["old"].encode(), C.byref(st), C.c_uint(0),
        ids.ctypes.data_as(C.POINTER(C.c_int32)), C.c_int(1), None, C.c_int(0), C.byref(n),
        None, None, None)
    assert rc == 0 and n.value == 1
    assert _sgm_file(dirs["old"]) == _sgm_file(dirs["default"])
