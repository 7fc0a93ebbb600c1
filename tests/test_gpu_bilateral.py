"""The four forms of the joint bilateral upsample (csrc/bilateral.hip) against
the CPU oracle (oracle.bilateral_upsample, the reference loop of
depth_optimizer.cc:957-1004 transcribed) on tests/bilateral_cases.py:

  bilateral_triangle_kernel<1|3>  context, kernel_size == 5       array_equal
  bilateral_table_kernel<1|3>     context, kernel_size <= 7       array_equal
  bilateral_kernel                context, kernel_size > 7        1e-5 max|want|
  bilateral_kernel                smvs_bilateral_upsample         1e-5 max|want|

tests/test_bilateral_cases_cpu.py shows without a GPU that the cases have the
properties they are here for.
"""
import functools

import numpy as np
import pytest

import bilateral_cases as bc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import smvs_amd
    if smvs_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on a GPU")
    return smvs_amd


@functools.lru_cache(maxsize=None)
def _want(case):
    """The oracle's map of a case: computed once, shared, read-only."""
    from oracle import pyoracle
    img, dm = bc.inputs(case)
    want = pyoracle.bilateral_upsample(dm, bc.to_float(img), case.sigma, case.kernel_size)
    want.setflags(write=False)
    return want


def _ids(cases):
    return [c.name for c in cases]


def _in_context(hip, case, img=None, dm=None):
    if img is None:
        img, dm = bc.inputs(case)
    ctx = hip.ViewContext(case.w, case.h, 1)
    try:
        ctx.upload_image(-1, img)
        return ctx.sgm_init_depth(dm, case.sigma, case.kernel_size)
    finally:
        ctx.close()


def _assert_same_bits(got, want):
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, "%d of %d differ; first at %s: got %r want %r" % (
        bad.size, got.size, np.unravel_index(bad[0], got.shape), got.flat[bad[0]], want.flat[bad[0]])


# -------------------------------------------------- a. byte-guided, bit for bit
BYTE_GUIDED = [(c, form) for c in bc.CASES if c.kernel_size <= 7
               for form in (("triangle", "compressed") if c.kernel_size == 5 else ("compressed",))]


@pytest.mark.parametrize("case,form", BYTE_GUIDED,
                         ids=["%s-%s" % (c.name, f) for c, f in BYTE_GUIDED])
def test_byte_guided_forms_are_the_oracle_bit_for_bit(hip, oracle, monkeypatch, case, form):
    """smvs_ctx_sgm_init_depth with the colour weights from the host's tables:
    kernel_size 5 as the triangle of all byte pairs and (SMVS_BILATERAL=
    compressed) as the compressed table, every other window up to 7 as the
    compressed table.  Every pixel is compared, the ones whose weight sum is
    subnormal or underflows (the contrast case) among them."""
    monkeypatch.delenv("SMVS_BILATERAL", raising=False)
    if form == "compressed" and case.kernel_size == 5:
        monkeypatch.setenv("SMVS_BILATERAL", "compressed")
    try:
        got = _in_context(hip, case)
    finally:
        monkeypatch.delenv("SMVS_BILATERAL", raising=False)
    _assert_same_bits(got, _want(case))
    if case.kind == "contrast" and case.channels == 3:
        img, dm = bc.inputs(case)
        cls = bc.classify(*bc.weight_sums(dm, bc.to_float(img), case.sigma, case.kernel_size))
        assert (got[cls["subnormal"]] > 0).all() and (got[cls["underflow"]] == 0).all()


# ---------------------------------------------- b. exponentials on the device
# Not on the contrast pair: its weights are subnormal, and one ulp of a
# subnormal weight (the device's exponential is exp in double rounded once, the
# oracle's is glibc's expf) is a relative error of up to 2^-5 in a weight sum
# of a few such taps -- far beyond any bound meant for 24-bit weights.  The byte
# -guided forms above, which take the host's own weights, cover those pixels.
DEVICE_EXP = [c for c in bc.CASES if c.kind != "contrast"]


def _assert_device_exp(got, want):
    """The bound of test_bilateral_upsample_matches_oracle."""
    assert np.array_equal(got == 0, want == 0)
    worst = float(np.max(np.abs(got - want)))
    scale = float(np.max(np.abs(want)))
    print("max |got - want| = %.3e = %.3e max|want|, %d ulp"
          % (worst, worst / scale if scale > 0 else 0.0, int(bc.ulps(got, want).max())))
    assert worst <= 1e-5 * scale


@pytest.mark.parametrize("case", DEVICE_EXP, ids=_ids(DEVICE_EXP))
def test_stand_alone_upsample_matches_oracle(hip, oracle, case):
    """smvs_bilateral_upsample: float guidance, bilateral_kernel."""
    img, dm = bc.inputs(case)
    got = hip.bilateral_upsample(dm, bc.to_float(img), case.sigma, case.kernel_size)
    _assert_device_exp(got, _want(case))


@pytest.mark.parametrize("case", [c for c in DEVICE_EXP if c.kernel_size > 7],
                         ids=_ids([c for c in DEVICE_EXP if c.kernel_size > 7]))
def test_generic_kernel_inside_a_context_matches_oracle(hip, oracle, case):
    """kernel_size > 7 has no table: bilateral_kernel on the context's float
    image -- and that image is the bytes over 255, so the stand-alone entry
    gives the same bits."""
    img, dm = bc.inputs(case)
    got = _in_context(hip, case)
    _assert_device_exp(got, _want(case))
    alone = hip.bilateral_upsample(dm, bc.to_float(img), case.sigma, case.kernel_size)
    _assert_same_bits(got, alone)


# -------------------------------------- c. second trip of the persistent grid
@pytest.mark.parametrize("case", bc.SECOND_TRIP, ids=_ids(bc.SECOND_TRIP))
def test_triangle_form_second_trip_of_the_persistent_grid(hip, oracle, case):
    """bilateral_triangle_kernel: one workgroup of 1,024 lanes per CU, pix +=
    gridDim.x * 1024 -- more pixels than one trip covers."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert case.w * case.h > 1024 * cus, \
        "this device's grid covers %d x %d in one trip: the test needs a larger image" % (case.w, case.h)
    _assert_same_bits(_in_context(hip, case), _want(case))


# ------------------------------------------------- d. one context, many calls
def test_one_context_through_forms_and_map_sizes(hip, oracle, monkeypatch):
    """bil_tri, bil_lut, byte_stage, sgm_lowres and the pinned staging buffer
    (reallocated as the map grows) live as long as the context: a context that
    switches between forms and map sizes gives what a new one gives."""
    from smvs_amd._capi import SmvsError
    monkeypatch.delenv("SMVS_BILATERAL", raising=False)
    W, H = 45, 37
    img = bc.guide(W, H, 3, 77)
    maps = dict(small=bc.low(5, 4, 78, hole=False), large=bc.low(66, 58, 79),
                half=bc.low(23, 19, 80))
    calls = [("small", 5), ("large", 5), ("half", 3), ("half", 8), ("small", 5)]
    lib = hip._capi.load()

    def fresh(name, k):
        # (not a parked context with its tables and buffers in place)
        lib.smvs_release_workspaces()
        ctx = hip.ViewContext(W, H, 1)
        ctx.upload_image(-1, img)
        out = ctx.sgm_init_depth(maps[name], 5.0, k)
        ctx.close()
        return out

    want = [fresh(name, k) for name, k in calls]
    lib.smvs_release_workspaces()
    ctx = hip.ViewContext(W, H, 1)
    ctx.upload_image(-1, img)
    for (name, k), w in zip(calls, want):
        got = ctx.sgm_init_depth(maps[name], 5.0, k)
        _assert_same_bits(got, w)
        ref = oracle.bilateral_upsample(maps[name], bc.to_float(img), 5.0, k)
        assert (got != 0).any()
        if k <= 7:
            _assert_same_bits(got, ref)
        else:
            _assert_device_exp(got, ref)
    ctx.close()
    # the parked context comes back without its image
    again = hip.ViewContext(W, H, 1)
    with pytest.raises(SmvsError):
        again.sgm_init_depth(maps["small"])
    again.upload_image(-1, img)
    _assert_same_bits(again.sgm_init_depth(maps["small"]), want[0])
    again.close()


# --------------------------------- e. the stored-map conversion, ragged sizes
@pytest.mark.parametrize("channels", [3, 1])
def test_stored_map_conversion_at_a_ragged_size(hip, oracle, channels):
    """smvs_ctx_sgm_init_depth_mve (sgm_map_upload_kernel) on 23 x 19 under an
    anisotropic, off-centre inverse calibration: what smvs_ctx_sgm_init_depth
    gives for the host's conversion (depthmap_convert_conventions: float
    products and square root, 1 / len and the product in double)."""
    W, H, lw, lh = 45, 37, 23, 19
    img = bc.guide(W, H, channels, 91)
    f = np.float32
    # (depths in [2.8, 4.2): the ray lengths cross into the next binade, where
    # the embedding's rounding is coarser than the depth's -- values that do not
    # survive the round trip through the embedding unchanged)
    z = bc.low(lw, lh, 92) * f(1.4)
    fx, fy = f(0.9) * f(lw), f(1.3) * f(lw)
    inv = np.array([f(1) / fx, 0, -f(0.37) * f(lw) / fx,
                    0, f(1) / fy, -f(0.61) * f(lh) / fy,
                    0, 0, 1], dtype=np.float32)
    px = (np.arange(lw, dtype=np.float32) + f(0.5))[None, :]
    py = (np.arange(lh, dtype=np.float32) + f(0.5))[:, None]
    v = [inv[3 * r] * px + inv[3 * r + 1] * py + inv[3 * r + 2] for r in range(3)]
    assert all(a.dtype == np.float32 for a in v)
    length = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]).astype(np.float32)
    assert length.shape == (lh, lw) and length.max() > 1.2 * length.min()
    stored = (z.astype(np.float64) * length.astype(np.float64)).astype(np.float32)      # to MVE
    back = (stored.astype(np.float64) * (1.0 / length.astype(np.float64))).astype(np.float32)
    assert np.array_equal(back == 0, z == 0) and np.array_equal(stored == 0, z == 0)
    assert not np.array_equal(back, z)       # (the round trip is not the identity)
    ctx = hip.ViewContext(W, H, 1)
    ctx.upload_image(-1, img)
    want = ctx.sgm_init_depth(back)
    _assert_same_bits(want, oracle.bilateral_upsample(back, bc.to_float(img)))
    assert (want == 0).any() and (want > 0).any()
    _assert_same_bits(ctx.sgm_init_depth_mve(stored, inv), want)
    _assert_same_bits(ctx.sgm_init_depth_mve(z, inv, dm_is_z_depth=True), want)
    ctx.close()


# ---------------------------------------------------------------- f. refusals
def test_bad_arguments_are_refused(hip, oracle):
    """kernel_size < 0, sigma <= 0 and an empty map are argument errors on the
    stand-alone entry and on both context entries (SMVS_REQUIRE, ahead of any
    allocation or launch); the context works afterwards."""
    from smvs_amd._capi import SmvsError
    case = bc.CASES[0]
    img, dm = bc.inputs(case)
    ci = bc.to_float(img)
    inv = np.array([0.05, 0, -0.5, 0, 0.05, -0.4, 0, 0, 1], np.float32)
    ctx = hip.ViewContext(case.w, case.h, 1)
    ctx.upload_image(-1, img)
    bad = [dict(dm=dm, sigma=5.0, kernel_size=-1),
           dict(dm=dm, sigma=0.0, kernel_size=5),
           dict(dm=np.zeros((0, 5), np.float32), sigma=5.0, kernel_size=5),
           dict(dm=np.zeros((5, 0), np.float32), sigma=5.0, kernel_size=5)]
    for a in bad:
        with pytest.raises(SmvsError):
            hip.bilateral_upsample(a["dm"], ci, a["sigma"], a["kernel_size"])
        with pytest.raises(SmvsError):
            ctx.sgm_init_depth(a["dm"], a["sigma"], a["kernel_size"])
        with pytest.raises(SmvsError):
            ctx.sgm_init_depth_mve(a["dm"], inv, a["sigma"], a["kernel_size"])
    _assert_same_bits(ctx.sgm_init_depth(dm), _want(case))
    ctx.close()
