"""Node slopes from the SGM plane hypotheses (include/smvs_hip.h) on the device:
csrc/surface_planes.hip against the C++ host mirror and the numpy restatement
(tests/surface_planes_ref.py), bit for bit; the three C entries; the layers
above (DepthOptimizer::Options::init_slants, ReconSettings::init_slants)."""
import ctypes as C
import os

import numpy as np
import pytest

import bilateral_cases as bc
import surface_planes_ref as ref
from test_surface_planes_cpu import H, SCALES, SCRIPTS, W, rough_maps

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import smvs_amd
    if smvs_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on a GPU")
    return smvs_amd


@pytest.fixture(scope="module")
def host(hip):
    from smvs_amd import host as h
    h.load()
    return h


@pytest.fixture(scope="module")
def scene():
    from smvs_amd import synth
    return synth.pipeline_inputs("sphere", W, H, 2, flen=1.2)


@pytest.mark.parametrize("scale", SCALES)
def test_device_equals_host_mirror_and_restatement(host, scene, scale):
    """The maps and scripts of tests/test_surface_planes_cpu.py at the five init
    scales: 64 x 64 pixels per node (64 keys per lane in registers), 16 x 16, 8 x 8
    (one wave per node, 4 and 1 keys per lane), 4 x 4 and 2 x 2 (lane groups of 16
    and 4) -- every form of the kernel short of the re-reading one."""
    depth, plane = rough_maps(scale)
    cache = {}

    def run(ops):
        key = tuple(ops)
        if key not in cache:
            cache[key] = host.surface_script(scene, scale, ops, init_depth=depth,
                                             init_slant=plane, device=0)
        return cache[key]

    for ops in SCRIPTS:
        if scale - ops.count(2) < 0:
            continue
        ref.check_script(run, depth, plane, scale, ops)
        mirror = host.surface_script(scene, scale, ops, init_depth=depth, init_slant=plane)
        ref.same_surface(run(ops), mirror)
        assert run(ops)["valid_patches"] == int(mirror["patch_valid"].sum()) > 0


def test_patch_size_128_rereads_the_maps(host):
    """Scale 7 (the kernel form that keeps no keys in registers) at the smallest
    image that has a patch of 128 pixels."""
    from smvs_amd import synth
    w, h = 260, 258
    scn = synth.pipeline_inputs("sphere", w, h, 2, flen=1.2)
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    depth = (4.0 + 0.002 * xx + 0.001 * yy + 0.01 * rng.standard_normal((h, w))
             ).astype(np.float32)
    depth[::7, ::5] = 0.0
    plane = (0.002 + 0.001 * rng.standard_normal((h, w, 2))).astype(np.float32)
    plane[rng.random((h, w)) < 0.2] = np.nan
    got = host.surface_script(scn, 7, [], init_depth=depth, init_slant=plane, device=0)
    want, cs = ref.create(depth, plane, 7)
    ref.same_surface(got, want)
    assert got["npx"] == 1 and got["patch_valid"].sum() == 1 and (cs > 0).all()


def _mve_case(channels=3):
    """tests/test_gpu_bilateral.py's stored-map case: 45 x 37 guided, 23 x 19 map."""
    Wc, Hc, lw, lh = 45, 37, 23, 19
    img = bc.guide(Wc, Hc, channels, 91)
    f = np.float32
    z = bc.low(lw, lh, 92) * f(1.4)
    fx, fy = f(0.9) * f(lw), f(1.3) * f(lw)
    inv = np.array([f(1) / fx, 0, -f(0.37) * f(lw) / fx,
                    0, f(1) / fy, -f(0.61) * f(lh) / fy, 0, 0, 1], dtype=np.float32)
    px = (np.arange(lw, dtype=np.float32) + f(0.5))[None, :]
    py = (np.arange(lh, dtype=np.float32) + f(0.5))[:, None]
    v = [inv[3 * r] * px + inv[3 * r + 1] * py + inv[3 * r + 2] for r in range(3)]
    length = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]).astype(np.float32)
    stored = (z.astype(np.float64) * length.astype(np.float64)).astype(np.float32)
    back = (stored.astype(np.float64) * (1.0 / length.astype(np.float64))).astype(np.float32)
    return Wc, Hc, img, z, inv, stored, back


def test_slant_plane_of_a_context(hip):
    """smvs_ctx_sgm_init_slants against the numpy tap rule, behind each of the
    three uploads of the map; a new map, and a NULL, forget the plane."""
    from smvs_amd._capi import SmvsError
    Wc, Hc, img, z, inv, stored, back = _mve_case()
    assert (back == 0).any() and (back > 0).any()
    rng = np.random.default_rng(5)
    g = rng.standard_normal(back.shape + (2,)).astype(np.float32)
    g[2, 3, 0] = np.nan
    g[4, 1, 1] = -np.inf
    g[5, 5] = (-0.0, 0.0)
    want = ref.tap_plane(back, g, Wc, Hc)
    assert np.isnan(want).any() and np.isfinite(want).any()
    ctx = hip.ViewContext(Wc, Hc, 1)
    try:
        with pytest.raises(SmvsError) as e:
            ctx.sgm_init_slants(g)                     # no resident map
        assert e.value.status == -3                    # SMVS_ERR_STATE
        ctx.upload_image(-1, img)
        filtered = []
        for upload in (lambda: ctx.sgm_init_depth(back),
                       lambda: ctx.sgm_init_depth_mve(stored, inv),
                       lambda: ctx.sgm_init_depth_mve(z, inv, dm_is_z_depth=True)):
            filtered.append(upload())
            with pytest.raises(SmvsError) as e:        # the new map forgot the plane
                ctx.create_surface(2, planes=True)
            assert e.value.status == -3
            got = ctx.sgm_init_slants(g)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
            surf = ctx.create_surface(2, planes=True)
            assert np.array_equal(ctx.surface_slants().view(np.uint32), want.view(np.uint32))
            made, _ = ref.create(filtered[-1], want, 2)
            ref.same_surface(surf, made)
        with pytest.raises(SmvsError) as e:            # size mismatch
            ctx.sgm_init_slants(g[1:])
        assert e.value.status == -1                    # SMVS_ERR_INVALID
        d = np.ascontiguousarray(filtered[0])          # depth without slant
        assert ctx.lib.smvs_surface_create_planes(
            ctx.handle, 2, d.ctypes.data_as(C.POINTER(C.c_float)), None, None) == -1
        ctx.sgm_init_slants(None)
        with pytest.raises(SmvsError):
            ctx.create_surface(2, planes=True)
        # smvs_surface_create ends the rule: no plane on the surface any more
        ctx.create_surface(2)
        with pytest.raises(SmvsError):
            ctx.surface_slants()
    finally:
        ctx.close()


@pytest.mark.parametrize("init_scale", [6, 4, 3, 2, 1])
def test_the_old_entry_gives_the_parents_bytes(hip, host, oracle, init_scale):
    """tests/test_gpu_surface.py's test_device_surface_from_an_initial_depth_map
    inputs through smvs_surface_create and the fill behind a subdivision, on a
    context that has just held a surface with slants."""
    from smvs_amd import synth
    scn = synth.pipeline_inputs("sphere", 416, 300, 2, flen=1.2)
    h, w = 300, 416
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    rng = np.random.default_rng(init_scale)
    depth = (4.0 + 0.002 * xx + 0.001 * yy + 0.01 * rng.standard_normal((h, w))
             ).astype(np.float32)
    depth[:, w // 2:] += 0.8
    depth[40:90, 60:140] = 0.0
    depth[::7, ::5] = 0.0
    depth[200:, 300:] = 0.0
    plane = rough_maps(init_scale)[1]
    ctx = hip.ViewContext(w, h, 1)
    try:
        with_slants = ctx.create_surface(init_scale, depth=depth, slant=plane)
        got = ctx.create_surface(init_scale, depth=depth)
        # a context that never held slants, to the byte; the oracle as
        # tests/test_gpu_surface.py compares with it
        ref.same_surface(got, host.surface_script(scn, init_scale, [], init_depth=depth,
                                                  device=0))
        want = oracle.surface_script(scn, init_scale, [], init_depth=depth)
        assert np.array_equal(got["node_valid"], want["node_valid"])
        assert np.array_equal(got["patch_valid"], want["patch_valid"])
        assert np.array_equal(got["nodes"][got["node_valid"].astype(bool)],
                              want["nodes"][got["node_valid"].astype(bool)])
        m = got["node_valid"].astype(bool)
        assert not np.array_equal(with_slants["nodes"][m], got["nodes"][m])
        from smvs_amd._capi import check
        valid = C.c_int(0)
        check(ctx.lib.smvs_surface_subdivide(ctx.handle, None))
        check(ctx.lib.smvs_surface_fill_patches_from_depth(ctx.handle, C.byref(valid)))
        ref.same_surface(ctx.surface_download(),
                         host.surface_script(scn, init_scale, [2, 3], init_depth=depth))
    finally:
        ctx.close()


def _log(out):
    return [[e["scale"], e["iter"], e["newton_steps"], e["valid_patches"], e["cg_iterations"],
             int(e["active_patch_steps"])] for e in out["log"]]


def test_optimize_with_init_slants(host, monkeypatch):
    """DepthOptimizer::optimize at 320 x 240 with three neighbours, the SGM map
    truth[::2, ::2] and slants from its finite differences: the device-resident
    path (smvs_ctx_sgm_init_slants + smvs_surface_create_planes) against
    SMVS_HOST_SURGERY (Surface::slant_plane + Surface::create on the host) with
    the comparisons of tests/test_gpu_surface.py's last test; init_slants=False is
    a call without the keyword."""
    from smvs_amd import synth
    inputs = synth.pipeline_inputs("sphere", 320, 240, 3, flen=1.2)
    truth = np.asarray(inputs["truth"], dtype=np.float32)
    sgm = np.where(truth > 0, truth, 0).astype(np.float32)[::2, ::2].copy()
    gx = np.zeros_like(sgm)
    gy = np.zeros_like(sgm)
    gx[:, :-1] = sgm[:, 1:] - sgm[:, :-1]
    gy[:-1, :] = sgm[1:, :] - sgm[:-1, :]
    slant = np.stack([gx, gy], axis=-1)
    edge = np.zeros(sgm.shape, bool)
    edge[:, :-1] |= ~((sgm[:, 1:] > 0) & (sgm[:, :-1] > 0))
    edge[:-1, :] |= ~((sgm[1:, :] > 0) & (sgm[:-1, :] > 0))
    edge[:, -1] = edge[-1, :] = True
    slant[edge] = np.nan
    assert np.isfinite(slant).mean() > 0.2
    kw = dict(regularization=0.01, num_iterations=4, min_scale=2, sgm_depth=sgm)
    monkeypatch.delenv("SMVS_HOST_SURGERY", raising=False)
    dev = host.optimize(inputs, sgm_slant=slant, init_slants=True, **kw)
    off = host.optimize(inputs, sgm_slant=slant, init_slants=False, **kw)
    plain = host.optimize(inputs, **kw)
    monkeypatch.setenv("SMVS_HOST_SURGERY", "1")
    surgery = host.optimize(inputs, sgm_slant=slant, init_slants=True, **kw)
    monkeypatch.delenv("SMVS_HOST_SURGERY")
    assert _log(dev) == _log(surgery), (_log(dev), _log(surgery))
    assert len(_log(dev)) >= 3
    assert np.array_equal(dev["depth"].view(np.uint32), surgery["depth"].view(np.uint32))
    assert (dev["depth"] > 0).mean() > 0.2
    assert _log(off) == _log(plain)
    assert np.array_equal(off["depth"].view(np.uint32), plain["depth"].view(np.uint32))
    # (the option does something: another start, another run)
    assert not np.array_equal(dev["depth"], plain["depth"])


def test_reconstruct_scene_with_init_slants(hip, host, tmp_path):
    """ReconSettings::init_slants on the small written scene of
    tests/test_gpu_sgm_refine.py.  The scene driver keeps no intermediate surface,
    so the initial nodes are rebuilt from what the run stored: the context entries
    fed with the view's smvs-sgm and smvs-sgm-slant embeddings (the calls
    DepthOptimizer makes) against smvs_host_surface_script_planes."""
    from smvs_amd import mve_scene
    from test_gpu_sgm_refine import PLANES, _spread_ring_inputs
    from test_gpu_parity import _inverse_calibration
    inputs = _spread_ring_inputs()
    path = str(tmp_path / "scene")
    os.makedirs(path)
    mve_scene.write_scene(path, inputs)
    run = dict(view_ids=[0], num_neighbors=3, min_neighbors=2, output_scale=2,
               sgm_num_steps=PLANES, sgm_photo_radius=2, sgm_refine_sweeps=2)
    view = os.path.join(path, "views", "view_0000.mve")
    done, skipped, _ = host.reconstruct_scene(path, **run)
    assert done == [0] and skipped == 0
    plain = mve_scene.load_mvei(os.path.join(view, "smvs-B0.mvei"))
    done, skipped, _ = host.reconstruct_scene(path, init_slants=True, force_recon=True, **run)
    assert done == [0] and skipped == 0           # (the stored smvs-sgm + slant are reused)
    got = mve_scene.load_mvei(os.path.join(view, "smvs-B0.mvei"))
    assert (got > 0).mean() > 0.2 and not np.array_equal(got, plain)
    stored = mve_scene.load_mvei(os.path.join(view, "smvs-sgm.mvei"))
    slant = mve_scene.load_mvei(os.path.join(view, "smvs-sgm-slant.mvei"))
    assert slant.shape == stored.shape + (2,) and slant.any()
    h, w = np.asarray(inputs["images"][0]).shape[:2]
    ctx = hip.ViewContext(w, h, 1)
    try:
        ctx.upload_image(-1, inputs["images"][0])
        inv = _inverse_calibration(inputs["cams"][0].flen, stored.shape[1], stored.shape[0])
        filtered = ctx.sgm_init_depth_mve(stored, inv)
        plane = ctx.sgm_init_slants(slant)
        # (the tap reads L only for its sign, which the conversion keeps)
        want_plane = ref.tap_plane(stored, slant, w, h)
        assert np.array_equal(plane.view(np.uint32), want_plane.view(np.uint32))
        surf = ctx.create_surface(4, planes=True)
    finally:
        ctx.close()
    sel = dict(inputs, cams=inputs["cams"][:2], images=inputs["images"][:2],
               view_ids=inputs["view_ids"][:2])
    mirror = host.surface_script(sel, 4, [], init_depth=filtered, init_slant=plane)
    ref.same_surface(surf, mirror)
    assert surf["patch_valid"].sum() > 0
