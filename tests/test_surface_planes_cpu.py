"""Node slopes from the SGM plane hypotheses (include/smvs_hip.h), host side: the
C++ host mirror (csrc/host/surface.cc, which compiles the per-node arithmetic
the device kernel compiles, csrc/host/surface_math.h) against the numpy
restatement tests/surface_planes_ref.py, the units and the sign of the rule on
an exact plane, the tap rule, and the error paths.  No device involved."""
import ctypes as C

import numpy as np
import pytest

import surface_planes_ref as ref

W, H = 416, 300
SCALES = [6, 4, 3, 2, 1]
SCRIPTS = [[], [1], [2, 3], [1, 2, 3, 4]]


@pytest.fixture(scope="module")
def host():
    from smvs_amd import host as h
    h.load()
    return h


@pytest.fixture(scope="module")
def scene():
    from smvs_amd import synth
    return synth.pipeline_inputs("sphere", W, H, 2, flen=1.2)


def plane_map():
    """D = 4 + x/256 + y/512, exact in float, and its slant plane."""
    yy, xx = np.mgrid[0:H, 0:W]
    depth = (4.0 + xx / 256.0 + yy / 512.0).astype(np.float32)
    assert np.array_equal(depth.astype(np.float64), 4.0 + xx / 256.0 + yy / 512.0)
    plane = np.empty((H, W, 2), np.float32)
    plane[..., 0] = 1.0 / 256.0
    plane[..., 1] = 1.0 / 512.0
    return depth, plane


def rough_maps(seed):
    """The depth map of tests/test_gpu_surface.py (a step, a hole, scattered
    zeros) and a slant plane with everything the rule distinguishes."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    rng = np.random.default_rng(seed)
    depth = (4.0 + 0.002 * xx + 0.001 * yy + 0.01 * rng.standard_normal((H, W))
             ).astype(np.float32)
    depth[:, W // 2:] += 0.8
    depth[40:90, 60:140] = 0.0
    depth[::7, ::5] = 0.0
    depth[200:, 300:] = 0.0
    plane = np.empty((H, W, 2), np.float32)
    plane[..., 0] = 0.002 + 0.001 * rng.standard_normal((H, W))
    plane[..., 1] = 0.001 + 0.001 * rng.standard_normal((H, W))
    # scattered "no slant" pixels, one or both components, and infinities
    plane[rng.random((H, W)) < 0.2] = np.nan
    plane[rng.random((H, W)) < 0.03, 0] = np.nan
    plane[rng.random((H, W)) < 0.03, 1] = np.nan
    plane[rng.random((H, W)) < 0.01, 0] = np.inf
    plane[rng.random((H, W)) < 0.01, 1] = -np.inf
    # ties between -0.0 and +0.0, and between equal values
    tie = np.where((xx[260:300, 0:100] + yy[260:300, 0:100]) % 2 == 0, 0.0, -0.0)
    plane[260:300, 0:100, 0] = tie
    plane[260:300, 0:100, 1] = -tie
    plane[0:30, 330:400] = np.float32(0.00390625)
    # a block of 160 x 160 without any slant where the depth is valid ...
    plane[95:255, 140:300] = np.nan
    # ... except single pixels far apart: windows with exactly one slant
    for (y, x) in ((180, 240), (120, 170), (121, 250), (230, 200)):
        plane[y, x] = (0.003, -0.002)
    return depth, plane


def test_units_and_sign_on_an_exact_plane(host, scene):
    """On D = 4 + x/256 + y/512 with P = (1/256, 1/512) every created node whose
    window lies inside the image has dx = ps/256, dy = ps/512, dxy = 0 exactly,
    and the surface's depth map has the plane's pixel differences to 4 ulps of
    the depth; the slant-free rule starts with half the slope and misses that."""
    depth, plane = plane_map()
    for scale in SCALES:
        ps = 1 << scale
        got = host.surface_script(scene, scale, [], init_depth=depth, init_slant=plane)
        free = host.surface_script(scene, scale, [], init_depth=depth)
        stride = got["npx"] + 1
        ids = np.flatnonzero(got["node_valid"])
        x = (ids % stride) * ps + got["start_x"]
        y = (ids // stride) * ps + got["start_y"]
        inside = (x - ps // 2 >= 0) & (x + ps // 2 <= W) & (y - ps // 2 >= 0) & (y + ps // 2 <= H)
        assert inside.sum() >= 6
        n = got["nodes"][ids[inside]]
        assert np.all(n[:, 1] == ps / 256.0) and np.all(n[:, 2] == ps / 512.0)
        assert np.all(n[:, 3] == 0.0)
        # the reference's rule: differences of quadrant minima ps/2 apart
        f = free["nodes"][ids[inside]]
        assert np.all(f[:, 1] == ps / 512.0) and np.all(f[:, 2] == ps / 1024.0)

    bound = 4.0 * 2.0 ** -21
    for scale in (4, 2):
        errs = []
        for init_slant in (plane, None):
            dm, _ = host.surface_maps(scene, scale, init_depth=depth, init_slant=init_slant,
                                      device=None)
            ok = dm > 0
            assert ok.mean() > 0.5
            dx = (dm[:, 1:].astype(np.float64) - dm[:, :-1])[ok[:, 1:] & ok[:, :-1]]
            dy = (dm[1:, :].astype(np.float64) - dm[:-1, :])[ok[1:, :] & ok[:-1, :]]
            errs.append(max(np.abs(dx - 1.0 / 256.0).max(), np.abs(dy - 1.0 / 512.0).max()))
        print("scale %d: max slope error with slants %.3g, without %.3g (bound %.3g)"
              % (scale, errs[0], errs[1], bound))
        assert errs[0] <= bound
        assert errs[1] > 1e-3 > bound


@pytest.mark.parametrize("scale", SCALES)
def test_host_mirror_equals_the_numpy_restatement(host, scene, scale):
    depth, plane = rough_maps(scale)
    cache = {}

    def run(ops):
        key = tuple(ops)
        if key not in cache:
            cache[key] = host.surface_script(scene, scale, ops, init_depth=depth,
                                             init_slant=plane)
        return cache[key]

    for ops in SCRIPTS:
        if scale - ops.count(2) < 0:
            continue
        cs = ref.check_script(run, depth, plane, scale, ops)
    # the inputs reach every class of the rule at this scale
    created = cs[cs >= 0]
    assert (created == 0).any(), "no created node without a slant"
    assert (created % 2 == 1).any(), "no created node with an odd number of slants"
    assert ((created % 2 == 0) & (created >= 2)).any(), "no created node with an even number"
    assert run([])["patch_valid"].sum() > 0


@pytest.mark.parametrize("scale", SCALES)
def test_existence_and_f_are_the_slant_free_run(host, scene, scale):
    depth, plane = rough_maps(scale)
    for ops in ([], [2, 3]):
        if scale - ops.count(2) < 0:
            continue
        got = host.surface_script(scene, scale, ops, init_depth=depth, init_slant=plane)
        free = host.surface_script(scene, scale, ops, init_depth=depth)
        assert np.array_equal(got["node_valid"], free["node_valid"])
        assert np.array_equal(got["patch_valid"], free["patch_valid"])
        if not ops:     # (a subdivision evaluates the patches: f then depends on the slopes)
            m = got["node_valid"].astype(bool)
            assert np.array_equal(got["nodes"][m, 0].view(np.uint64),
                                  free["nodes"][m, 0].view(np.uint64))
            assert not np.array_equal(got["nodes"][m, 1:], free["nodes"][m, 1:])
        # an all-NaN plane: the slant-free nodes to the byte
        nan = np.full((H, W, 2), np.nan, np.float32)
        none = host.surface_script(scene, scale, ops, init_depth=depth, init_slant=nan)
        ref.same_surface(none, free)


@pytest.mark.parametrize("size,dm", [((23, 19), (12, 10)), ((22, 18), (11, 9))])
def test_tap_rule(host, size, dm):
    (w, h), (dw, dh) = size, dm
    rng = np.random.default_rng(w)
    low = (3.0 + rng.random((dh, dw))).astype(np.float32)
    low[rng.random((dh, dw)) < 0.25] = 0.0
    low[0, 0] = -1.0
    low[dh - 1, dw - 1] = np.nan
    g = rng.standard_normal((dh, dw, 2)).astype(np.float32)
    g[1, 2, 0] = np.nan
    g[2, 1, 1] = np.inf
    g[3, 3] = (-0.0, 0.0)
    got = host.slant_plane(low, g, w, h)
    want = ref.tap_plane(low, g, w, h)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    none = np.isnan(got[..., 0])
    assert np.array_equal(none, np.isnan(got[..., 1]))
    assert np.all(got.view(np.uint32)[none] == 0x7FC00000)
    # pixels whose tap has no depth, and pixels that have a slant
    sx = np.clip(np.float32(dw) / np.float32(w) * np.arange(w, dtype=np.float32), 0,
                 dw - 1).astype(int)
    sy = np.clip(np.float32(dh) / np.float32(h) * np.arange(h, dtype=np.float32), 0,
                 dh - 1).astype(int)
    no_depth = ~(low[sy[:, None], sx[None, :]] > 0)
    assert no_depth.any() and np.all(none[no_depth]) and (~none).any()


def test_keys_order_like_the_floats(host):
    v = np.array([-np.inf, -3.5, -1e-40, -0.0, 0.0, 1e-40, 2.0, np.inf], np.float32)
    k = ref.slant_key(v)
    assert np.all(k[1:] > k[:-1])
    assert np.array_equal(ref.slant_from_key(k).view(np.uint32), v.view(np.uint32))


def test_error_paths_come_before_any_device_call(host, scene):
    from smvs_amd import _capi, build as hip_build
    hip_build.build()
    lib = _capi.load()
    # the C ABI: argument errors are status codes
    assert lib.smvs_ctx_sgm_init_slants(None, None, 0, 0, None) == -1
    assert lib.smvs_surface_create_planes(None, 4, None, None, None) == -1
    assert lib.smvs_surface_slants(None, None) == -1
    for name in ("smvs_ctx_sgm_init_slants", "smvs_surface_create_planes",
                 "smvs_surface_slants"):
        assert name in _capi.declared_symbols()

    # DepthOptimizer::Options::init_slants: never silently ignored.  (Each message
    # is the option's own: the constructor has not reached smvs_ctx_create.)
    small = dict(scene)
    sgm = np.full((H // 2, W // 2), 5.0, np.float32)
    slant = np.zeros((H // 2, W // 2, 2), np.float32)
    with pytest.raises(_capi.SmvsError, match="init_slants needs use_sgm"):
        host.optimize(small, init_slants=True)
    with pytest.raises(_capi.SmvsError, match="init_slants needs use_sgm"):
        host.optimize(small, sgm_slant=slant, init_slants=True)
    for bad in (None, slant[..., 0], np.zeros((H // 2, W // 2, 3), np.float32), slant[1:],
                slant[:, 1:]):
        with pytest.raises(_capi.SmvsError, match="init_slants needs an smvs-sgm-slant"):
            host.optimize(small, sgm_depth=sgm, sgm_slant=bad, init_slants=True)
    hlib = host.load()
    rc = hlib.smvs_host_optimize_planes(None, None, C.c_int(0), None, None, C.c_int(0),
                                        C.c_int(0), None, None, C.c_int(0), C.c_int(0),
                                        C.c_int(0), None, C.c_uint(4), None, None, None)
    assert rc == -1 and b"unknown flag" in hlib.smvs_host_last_error()

    # the surface entries of the host API
    depth, plane = plane_map()
    with pytest.raises(ValueError):
        host.surface_script(scene, 4, [], init_slant=plane)
    with pytest.raises(ValueError):
        host.surface_script(scene, 4, [], init_depth=depth, init_slant=plane[:, :, 0])
    with pytest.raises(ValueError):
        host.surface_maps(scene, 4, init_slant=plane)
    rc = hlib.smvs_host_surface_script_planes_device(None, None, None, C.c_int(4), None,
                                                     C.c_int(0), C.c_int(1), C.c_int(0), None,
                                                     None, None, None)
    assert rc == -1 and b"are required" in hlib.smvs_host_last_error()
    rc = hlib.smvs_host_surface_maps_planes(None, None, C.c_int(0), None, None, None,
                                            C.c_int(4), C.c_int(0), None, None)
    assert rc == -1 and b"are required" in hlib.smvs_host_last_error()
    with pytest.raises(ValueError):
        host.slant_plane(np.zeros((4, 4), np.float32), np.zeros((4, 4), np.float32), 8, 8)

    # the scene driver: init_slants without the refinement sweeps
    with pytest.raises(ValueError, match="sgm_refine_sweeps"):
        host.reconstruct_scene("/nonexistent", init_slants=True, sgm_refine_sweeps=0)
    st = host.ReconSettings(b"undistorted", 1.0, 2, 0, 1, 0, 0, 0, 0.0, 0.0, 1, 6, 3, 0, 1, 2,
                            -1, 1700000)
    for entry, flags, text in ((hlib.smvs_host_reconstruct_scene_planes, 32,
                                b"init_slants needs sgm_refine_sweeps"),
                               (hlib.smvs_host_reconstruct_scene_planes, 64, b"unknown flag"),
                               (hlib.smvs_host_reconstruct_scene_refine, 32, b"unknown flag")):
        rc = entry(b"/nonexistent", C.byref(st), C.c_uint(flags), C.c_int(128), C.c_int(0),
                   C.c_int(2), C.c_int(0), C.c_float(0.95), C.c_int(2), None, None, None, None,
                   None, C.c_int(0), None, C.c_int(0), None, None, None, None)
        assert rc != 0 and text in hlib.smvs_host_last_error(), (flags, text)
