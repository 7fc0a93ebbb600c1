"""The device shading preparation (smvs_ctx_prepare_shading: the main view's
StereoView::initialize_linear, lib/stereo_view.cc:64-84, as one kernel) against
the host mirror's planes and, without gamma, against numpy and the oracle's
quadratic fit.  The device path promises the host's bits, so every comparison is
np.array_equal / byte equality."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INVALID, STATE = -1, -3

# 3: one interior pixel; 4; 255 / 256 / 257 / 259: the halo column on either
# side of the 256-column workgroup boundary; 515: two full tiles and a partial one
WIDTHS = (3, 4, 255, 256, 257, 259, 515)
# GRAD_ROWS of csrc/scale.hip is 8 rows per workgroup: 3 (one interior row),
# GRAD_ROWS, GRAD_ROWS + 1 (a tile of one row), 2 * GRAD_ROWS + 3
HEIGHTS = (3, 8, 9, 19)


@pytest.fixture(scope="module")
def hip():
    import smvs_amd
    if smvs_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on a GPU")
    return smvs_amd


@pytest.fixture(scope="module")
def lut():
    from smvs_amd import host
    return host.gamma_inv_srgb_lut()


def _contents(w, h, c):
    rng = np.random.default_rng(1000 * w + 10 * h + c)
    ys, xs = np.mgrid[0:h, 0:w]
    yield "random", rng.integers(0, 256, (h, w, c)).astype(np.uint8)
    yield "all0", np.zeros((h, w, c), np.uint8)
    yield "all255", np.full((h, w, c), 255, np.uint8)
    # every byte value along a row (where the row is long enough), another
    # phase per channel
    ramp = (xs % 256).astype(np.uint8)
    yield "ramp", np.stack([np.roll(ramp, 85 * k, axis=1) for k in range(c)], axis=2).copy()
    for period in (1, 2):
        board = ((((xs // period) + (ys // period)) & 1) * 255).astype(np.uint8)
        yield "checker%d" % period, np.repeat(board[:, :, None], c, axis=2).copy()


def _numpy_shading(img):
    f = img.astype(np.float32) / np.float32(255)
    if img.shape[2] == 1:
        return f[:, :, 0]
    return f[:, :, 0] * np.float32(0.21) + f[:, :, 1] * np.float32(0.72) \
        + f[:, :, 2] * np.float32(0.07)


@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("h", HEIGHTS)
def test_planes_equal_the_hosts(hip, oracle, lut, w, h):
    from smvs_amd import device, host
    ctx = device.ViewContext(w, h, 1)
    try:
        for c in (1, 3):
            for name, img in _contents(w, h, c):
                ctx.upload_image(-1, img)
                for gamma in (False, True):
                    ctx.prepare_shading(lut if gamma else None)
                    shading, grad = ctx.download_shading()
                    want_s, want_g = host.shading_planes(img, gamma=gamma)
                    what = (name, c, gamma)
                    assert np.array_equal(shading, want_s), what
                    assert np.array_equal(grad, want_g), what
                    if not gamma:
                        # independently of the host mirror
                        assert np.array_equal(shading, _numpy_shading(img)), what
                        assert np.array_equal(
                            grad, oracle.gradients_and_hessian(shading)[0]), what
                    elif c == 1:
                        assert np.array_equal(shading, lut[img[:, :, 0]]), what
    finally:
        ctx.close()


def test_a_pending_upload_is_materialised_by_the_entry(hip, lut):
    """640 x 600 x 3 is just over the 1 MiB from which smvs_ctx_upload_image_async
    only enqueues the transfer: nothing between it and prepare_shading converts
    the image, so the entry must"""
    from smvs_amd import device, host
    w, h = 640, 600
    assert w * h * 3 >= 1 << 20
    img = np.random.default_rng(5).integers(0, 256, (h, w, 3)).astype(np.uint8)
    ctx = device.ViewContext(w, h, 1)
    try:
        ctx.upload_image_async(-1, img)
        ctx.prepare_shading(lut)
        shading, grad = ctx.download_shading()
    finally:
        ctx.close()
    want_s, want_g = host.shading_planes(img, gamma=True)
    assert np.array_equal(shading, want_s) and np.array_equal(grad, want_g)


def test_prepared_planes_replace_uploaded_ones(hip):
    from smvs_amd import device, host
    w, h = 259, 19
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    other_s = rng.random((h, w), dtype=np.float32)
    other_g = rng.random((h, w, 2), dtype=np.float32)
    ctx = device.ViewContext(w, h, 1)
    try:
        ctx.upload_image(-1, img)
        ctx.upload_shading(other_s, other_g)
        got_s, got_g = ctx.download_shading()
        assert np.array_equal(got_s, other_s) and np.array_equal(got_g, other_g)
        ctx.prepare_shading()
        got_s, got_g = ctx.download_shading()
    finally:
        ctx.close()
    want_s, want_g = host.shading_planes(img)
    assert np.array_equal(got_s, want_s) and np.array_equal(got_g, want_g)
    assert not np.array_equal(got_s, other_s)


def test_no_main_image_is_an_argument_error(hip, lut):
    from smvs_amd import _capi, device, host
    ctx = device.ViewContext(64, 48, 1)
    try:
        # a neighbour's image is not the main view's
        ctx.upload_image(0, np.zeros((48, 64, 3), np.uint8))
        for table in (None, lut):
            with pytest.raises(_capi.SmvsError, match="no image") as err:
                ctx.prepare_shading(table)
            assert err.value.status == INVALID
            with pytest.raises(_capi.SmvsError) as err:
                ctx.download_shading()
            assert err.value.status == STATE
        # the context still works
        ctx.upload_image(-1, np.full((48, 64, 3), 255, np.uint8))
        ctx.prepare_shading(lut)
        shading, grad = ctx.download_shading()
        want_s, want_g = host.shading_planes(np.full((48, 64, 3), 255, np.uint8), gamma=True)
        assert np.array_equal(shading, want_s) and np.array_equal(grad, want_g)
        assert np.all(shading == lut[255] * np.float32(0.21) + lut[255] * np.float32(0.72)
                      + lut[255] * np.float32(0.07))
    finally:
        ctx.close()


@pytest.mark.parametrize("gamma", [False, True])
def test_optimize_is_the_same_with_the_planes_from_the_device(hip, gamma):
    """host.optimize with -S: depth, normals, lighting and the log (all but the
    wall times) of the run whose shading planes come from the device equal the
    run with the host's, the pipeline being run-to-run identical"""
    from smvs_amd import host, synth
    rng = np.random.default_rng(77)
    lighting = np.zeros(16); lighting[0] = 0.9
    lighting[1:4] = rng.uniform(-0.2, 0.2, 3)
    inputs = synth.pipeline_inputs("sphere", 320, 240, 3, lighting=lighting)
    runs = [host.optimize(inputs, use_shading=True, min_scale=2, gamma_correction=gamma,
                          device_shading_prep=flag) for flag in (False, True)]
    a, b = runs
    assert a["lighting"] is not None and np.isfinite(a["depth"]).any()
    assert np.array_equal(a["depth"], b["depth"], equal_nan=True)
    assert np.array_equal(a["normals"], b["normals"], equal_nan=True)
    assert np.array_equal(a["lighting"], b["lighting"])
    assert len(a["log"]) == len(b["log"]) > 0
    for la, lb in zip(a["log"], b["log"]):
        assert {k: v for k, v in la.items() if k != "loop_seconds"} \
            == {k: v for k, v in lb.items() if k != "loop_seconds"}


def test_scene_option_gives_the_host_paths_files(hip, tmp_path):
    """reconstruct_scene -S --gamma-srgb on the 384 x 256 scene of a reference
    view and three neighbours (with two, view selection keeps one and the view
    is skipped): the result embeddings with device_shading_prep are the host
    path's, byte for byte"""
    from smvs_amd import synth, host, mve_scene
    inputs = synth.pipeline_inputs("sphere", 384, 256, 3, flen=1.2)
    data = {}
    for flag in (False, True):
        d = str(tmp_path / ("device" if flag else "host"))
        os.makedirs(d)
        mve_scene.write_scene(d, inputs, container="png")
        done, skipped, secs, scale = host.reconstruct_scene(
            d, view_ids=[0], num_neighbors=3, min_neighbors=2, output_scale=2, input_scale=0,
            details=True, use_shading=True, gamma_correction=True, device_shading_prep=flag)
        assert scale == 0 and done == [0] and skipped == 0
        for name in ("smvs-S0.mvei", "smvs-S0N.mvei"):
            with open(os.path.join(d, "views", "view_0000.mve", name), "rb") as f:
                data[flag, name] = f.read()
    for name in ("smvs-S0.mvei", "smvs-S0N.mvei"):
        assert len(data[False, name]) > 1000 and data[False, name] == data[True, name], name
