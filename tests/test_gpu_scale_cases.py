"""smvs_ctx_set_scale on the case list of tests/scale_cases.py: every scale
0 .. 7 -- scale 7 is the run-time-width kernels, scale 0 the narrowest -- on
images whose widths and heights sit on either side of each predicate of
csrc/scale.hip's launch plan, on the seams of its tiles and on the smallest
images a context takes, grey and RGB, random and degenerate contents
(test_scale_cases_cpu.py shows that the list does that, and that a kernel
wrong in tap order, contraction, weight total, pass order, border or window
order would change some float of it).  Every comparison is an equality of
float32 BIT PATTERNS with the CPU oracle: -0 is not +0.  Then the context's
state between calls, the deferred conversion with a tail, and the refusals."""
import os

import numpy as np
import pytest

import scale_cases as sc  # tests/scale_cases.py
import scale_ref  # tests/scale_ref.py

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import smvs_amd
    if smvs_amd.device_count() < 1:
        pytest.fail("no HIP device")
    return smvs_amd


@pytest.fixture
def fused_switch():
    """Sets SMVS_SCALE_FUSED (read per set_scale call); restored afterwards."""
    old = os.environ.get("SMVS_SCALE_FUSED")

    def switch(value):
        os.environ["SMVS_SCALE_FUSED"] = value

    yield switch
    if old is None:
        os.environ.pop("SMVS_SCALE_FUSED", None)
    else:
        os.environ["SMVS_SCALE_FUSED"] = old


def _same_bits(got, want, what):
    d = sc.first_difference(got, want)
    assert d is None, "%s: %d floats differ, first at (y %d, x %d, channel %d): device %r (%#010x) " \
        "oracle %r (%#010x)" % (what, d[0], d[1][0], d[1][1], d[1][2], d[2],
                                scale_ref.bits(got)[d[1]], d[3], scale_ref.bits(want)[d[1]])


def _compare_view(ctx, view, want, what):
    """The planes of one view against the oracle's (gradient, Hessian)."""
    g, h = ctx.download_planes(view)
    _same_bits(g, want[0], what + " gradient of view %d" % view)
    if view >= 0:
        _same_bits(h, want[1], what + " hessian of view %d" % view)
    return g, h


@pytest.mark.parametrize("scale", sc.SCALES)
def test_planes_match_oracle_on_every_case(hip, oracle, fused_switch, scale):
    """Main view (no Hessian plane: the want_hess == false path) and
    neighbour 0 of one context per size, all contents through it; both forms
    of the y pass where the scale has a fused one."""
    forms = ("1", "0") if sc.has_fused(scale) else ("1",)
    for c in sc.CHANNELS:
        for w, h, group in sc.sizes(scale, c):
            ctx = hip.ViewContext(w, h, 1)
            try:
                for name, img in sc.images(w, h, c, group).items():
                    want = oracle.scale_planes(img, scale)
                    ctx.upload_image(-1, img)
                    ctx.upload_image(0, img)
                    for fused in forms:
                        fused_switch(fused)
                        ctx.set_scale(scale)
                        what = "scale %d %dx%dx%d %s fused=%s" % (scale, w, h, c, name, fused)
                        _compare_view(ctx, -1, want, what)
                        _compare_view(ctx, 0, want, what)
            finally:
                ctx.close()


def test_context_reuse(hip, oracle):
    """A neighbour re-uploaded at another size and channel count between two
    set_scale calls: its planes, the blur scratch and the byte staging buffer
    are reallocated (larger than anything the context held), the other views'
    planes recomputed in place; then the same set_scale twice."""
    rng = np.random.default_rng(5)
    main = rng.integers(0, 256, size=(61, 83, 3)).astype(np.uint8)
    sub0 = rng.integers(0, 256, size=(47, 70)).astype(np.uint8)
    sub1 = rng.integers(0, 256, size=(40, 64, 3)).astype(np.uint8)
    larger = rng.integers(0, 256, size=(120, 301)).astype(np.uint8)          # grey where it was RGB
    smaller = rng.integers(0, 256, size=(7, 9, 3)).astype(np.uint8)
    assert larger.size > main.size and sc.converter(larger.size)[1] != 0
    ctx = hip.ViewContext(83, 61, 2)
    try:
        ctx.upload_image(-1, main)
        ctx.upload_image(0, sub0)
        ctx.upload_image(1, sub1)
        views = {-1: main, 0: sub0, 1: sub1}
        for scale, replacement in ((6, None), (7, larger), (0, smaller)):
            if replacement is not None:
                ctx.upload_image(1, replacement)
                views[1] = replacement
            ctx.set_scale(scale)
            for view, img in views.items():
                _compare_view(ctx, view, oracle.scale_planes(img, scale), "scale %d" % scale)
        before = {view: ctx.download_planes(view) for view in views}
        ctx.set_scale(0)
        ctx.set_scale(0)
        for view, img in views.items():
            g, h = _compare_view(ctx, view, oracle.scale_planes(img, 0), "scale 0 again")
            _same_bits(g, before[view][0], "gradient of view %d after a repeated set_scale" % view)
            if view >= 0:
                _same_bits(h, before[view][1], "hessian of view %d after a repeated set_scale" % view)
    finally:
        ctx.close()


def test_async_ragged(hip, oracle):
    """1031 x 1025 grey bytes from page-locked memory: more than the 1 MiB from
    which smvs_ctx_upload_image_async defers the conversion, and 7 bytes beyond
    a multiple of 16, so the deferred byte_to_float16_kernel has a tail."""
    w, h = 1031, 1025
    assert w * h >= sc.ASYNC_FROM and sc.converter(w * h)[1] == 7
    rng = np.random.default_rng(1031)
    main = rng.integers(0, 256, size=(h, w)).astype(np.uint8)
    sub = rng.integers(0, 256, size=(h, w)).astype(np.uint8)
    ctx = hip.ViewContext(w, h, 1)
    try:
        ctx.upload_image_async(-1, main)
        ctx.upload_image_async(0, sub)
        ctx.set_scale(1)
        _compare_view(ctx, -1, oracle.scale_planes(main, 1), "async main")
        _compare_view(ctx, 0, oracle.scale_planes(sub, 1), "async neighbour")
    finally:
        ctx.close()


def test_refusals(hip, oracle):
    """Scales whose blur kernel has more than 64 weights, scales out of range
    and images a context does not take are refused before anything is launched:
    the planes of the last good scale stay downloadable and unchanged."""
    from smvs_amd._capi import SmvsError
    rng = np.random.default_rng(8)
    main = rng.integers(0, 256, size=(12, 14, 3)).astype(np.uint8)
    sub = rng.integers(0, 256, size=(9, 10)).astype(np.uint8)
    ctx = hip.ViewContext(14, 12, 1)
    try:
        ctx.upload_image(-1, main)
        ctx.upload_image(0, sub)
        # (the kernels of set_scale are counted in the context's class "misc")
        ctx.profile(True)
        ctx.profile_reset()
        ctx.set_scale(2)
        assert ctx.profile_get()["misc"][1] > 0
        ctx.profile_reset()
        want = {-1: oracle.scale_planes(main, 2), 0: oracle.scale_planes(sub, 2)}
        for scale in (8, 9, 10):
            assert sc.refused(scale)
            with pytest.raises(SmvsError, match="blur kernel too wide"):
                ctx.set_scale(scale)
            for view in (-1, 0):
                _compare_view(ctx, view, want[view], "after the refused scale %d" % scale)
        for scale in (-1, 11):
            with pytest.raises(SmvsError, match="scale out of range"):
                ctx.set_scale(scale)
        with pytest.raises(SmvsError, match="bad image"):
            ctx.upload_image(0, np.zeros((5, 2), np.uint8))             # 2 x 5
        with pytest.raises(SmvsError, match="bad image"):
            ctx.upload_image(0, np.zeros((5, 5, 2), np.uint8))          # two channels
        assert ctx.profile_get()["misc"][1] == 0
        ctx.profile(False)
        # the refused uploads left the neighbour's image alone
        ctx.set_scale(2)
        for view in (-1, 0):
            _compare_view(ctx, view, want[view], "after the refused uploads")
    finally:
        ctx.close()
