"""What makes tests/test_gpu_bilateral.py meaningful, checked on its inputs and
on the CPU oracle alone (no GPU): the size pairs really are sensitive to one
ulp of the tap scale, the contrast case really has subnormal and underflowed
weight sums, every other case keeps its sums normal (the 1e-5 bound of the
device-exponential paths rests on that), the holes really leave outputs
without taps, and the guidance images reach both ends of the byte range."""
import numpy as np
import pytest

import bilateral_cases as bc


def _ids(cases):
    return [c.name for c in cases]


ALL = bc.CASES + bc.SECOND_TRIP


def test_the_case_list_has_every_group():
    have = {(c.w, c.h, c.dm_w, c.dm_h, c.channels, c.kernel_size, c.sigma, c.kind) for c in bc.CASES}
    for ch in (3, 1):
        for size in [(45, 37, 23, 19), (45, 35, 15, 5), (66, 46, 39, 14), (64, 48, 64, 48),
                     (33, 29, 66, 58), (1100, 3, 550, 2)]:
            assert size + (ch, 5, 5.0, "holes") in have
        assert (7, 5, 3, 2, ch, 5, 5.0, "scatter") in have
        assert (3, 3, 1, 1, ch, 5, 5.0, "dense") in have
        for k in (0, 1, 3, 7, 8):
            assert (45, 37, 23, 19, ch, k, 5.0, "holes") in have
        assert (45, 37, 23, 19, ch, 5, 0.5, "scatter") in have
        assert (45, 37, 23, 19, ch, 5, 50.0, "holes") in have
        for kind in ("contrast", "zero", "dense"):
            assert (45, 37, 23, 19, ch, 5, 5.0, kind) in have
    for c in ALL:
        img, dm = bc.inputs(c)
        assert img.dtype == np.uint8 and dm.dtype == np.float32
        assert img.shape[:2] == (c.h, c.w) and dm.shape == (c.dm_h, c.dm_w)
        assert (img.ndim == 3 and img.shape[2] == 3) if c.channels == 3 else img.ndim == 2


def test_tap_flips_of_the_sensitive_pairs():
    """The figures the case list was chosen by: 15 / 45 and 5 / 35 (exact 1/3
    and 1/7 in the rationals, rounded up as floats) lose taps when the quotient
    is one ulp low, 39 / 66 and 14 / 46 when it is one ulp high."""
    assert bc.tap_flips(45, 15) == (14, 0)
    assert bc.tap_flips(35, 5) == (4, 0)
    assert bc.tap_flips(66, 39) == (0, 2)
    assert bc.tap_flips(46, 14) == (0, 1)
    # an exact ratio sits on the integers: every tap but the first moves when
    # the quotient is low, none when it is high
    assert bc.tap_flips(64, 64) == (63, 0)


def test_some_width_and_some_height_flips_in_each_direction():
    widths = [bc.tap_flips(c.w, c.dm_w) for c in bc.CASES]
    heights = [bc.tap_flips(c.h, c.dm_h) for c in bc.CASES]
    for flips in (widths, heights):
        assert any(f[0] > 0 for f in flips)
        assert any(f[1] > 0 for f in flips)


def test_tap_columns_are_the_oracles(oracle):
    """tap_columns() against the oracle itself: a map whose value is its own
    column (row) index, a window of one tap, a constant image."""
    for n, dm_n in [(45, 15), (66, 39), (35, 5), (46, 14), (33, 66), (1100, 550), (641, 321)]:
        dm = np.tile(np.arange(1, dm_n + 1, dtype=np.float32), (2, 1))
        out = oracle.bilateral_upsample(dm, np.zeros((3, n), np.float32), 5.0, 0)
        assert np.array_equal(out[0], bc.tap_columns(n, dm_n) + 1)
        out = oracle.bilateral_upsample(dm.T.copy(), np.zeros((n, 3), np.float32), 5.0, 0)
        assert np.array_equal(out[:, 0], bc.tap_columns(n, dm_n) + 1)


@pytest.mark.parametrize("channels", [3, 1])
def test_contrast_case_has_subnormal_and_underflowed_sums(oracle, channels):
    img, dm = bc.contrast_case()
    assert img.shape == (37, 45, 3) and dm.shape == (19, 23)
    if channels == 1:
        # the green channel alone: one channel differs by 255, exp(-50) -- normal
        # weights; the pair is in the list for the table's ends, not for its sums
        img = img[:, :, 1]
        sums, taps = bc.weight_sums(dm, bc.to_float(img), 5.0, 5)
        cls = bc.classify(sums, taps)
        assert cls["no_taps"].sum() > 0 and cls["normal"].sum() > 0
        assert np.array_equal(cls["no_taps"] | cls["normal"], np.ones_like(taps, bool))
        return
    sums, taps = bc.weight_sums(dm, bc.to_float(img), 5.0, 5)
    cls = bc.classify(sums, taps)
    counts = {k: int(v.sum()) for k, v in cls.items()}
    print(counts)
    assert counts["subnormal"] >= 50
    assert counts["underflow"] >= 30
    assert sum(counts.values()) == 45 * 37          # every pixel is in a class
    want = oracle.bilateral_upsample(dm, bc.to_float(img), 5.0, 5)
    assert (want[cls["subnormal"]] > 0).all()
    assert (want[cls["underflow"]] == 0).all()
    assert (want[cls["no_taps"]] == 0).all()
    assert (want[cls["normal"]] > 0).all()


@pytest.mark.parametrize("case", [c for c in ALL if c.kind not in ("contrast", "zero")],
                         ids=_ids([c for c in ALL if c.kind not in ("contrast", "zero")]))
def test_weight_sums_are_normal_outside_the_contrast_case(case):
    """1e-5 * max|want| for the paths that take exponentials on the device
    presumes weights with 24 bits: no sum near the subnormal range."""
    img, dm = bc.inputs(case)
    sums, taps = bc.weight_sums(dm, bc.to_float(img), case.sigma, case.kernel_size)
    assert (taps > 0).any()
    assert sums[taps > 0].min() >= 2.0 ** -120
    assert (sums[taps == 0] == 0).all()


@pytest.mark.parametrize("case", [c for c in ALL if bc.has_holes(c)],
                         ids=_ids([c for c in ALL if bc.has_holes(c)]))
def test_cases_with_holes_have_empty_and_filled_outputs(oracle, case):
    img, dm = bc.inputs(case)
    want = oracle.bilateral_upsample(dm, bc.to_float(img), case.sigma, case.kernel_size)
    assert (want == 0).any() and (want > 0).any()
    _, taps = bc.weight_sums(dm, bc.to_float(img), case.sigma, case.kernel_size)
    assert (want[taps == 0] == 0).all()
    # a filled output is a weighted mean of depths in [2, 3)
    assert (want[want != 0] >= 2).all() and (want[want != 0] <= 3).all()


def test_zero_and_dense_maps(oracle):
    for case in bc.CASES:
        img, dm = bc.inputs(case)
        if case.kind == "zero":
            assert not dm.any()
            assert not oracle.bilateral_upsample(dm, bc.to_float(img), case.sigma, case.kernel_size).any()
        if case.kind == "dense":
            assert (dm >= 2).all()
            assert (oracle.bilateral_upsample(dm, bc.to_float(img), case.sigma, case.kernel_size) >= 2).all()


def test_every_guidance_image_has_both_ends_of_the_byte_range():
    for case in ALL:
        img, _ = bc.inputs(case)
        assert img.min() == 0 and img.max() == 255, case.name


def test_maps_have_scattered_zeros_and_a_hole():
    dm = bc.low(23, 19, 7)
    x0, y0, x1, y1 = bc.hole_rect(23, 19)
    assert not dm[y0:y1, x0:x1].any()
    outside = np.ones(dm.shape, bool)
    outside[y0:y1, x0:x1] = False
    frac = np.mean(dm[outside] == 0)
    assert 0.1 < frac < 0.3
    assert (dm[dm != 0] >= 2).all() and (dm < 3).all()
