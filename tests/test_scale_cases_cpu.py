"""What makes tests/test_gpu_scale_cases.py meaningful, checked without a GPU:
the launch-plan mirror of tests/scale_cases.py has csrc/scale.hip's constants
(read from the source text: a retuned tile fails here instead of silently
untesting an edge), its case list sits on both sides of every predicate at
every scale, the float32 restatement tests/scale_ref.py and the CPU oracle
agree to the bit on every case (two readings of stereo_view.cc pinned against
each other before the device is judged), and each way of being subtly wrong
that scale_ref knows -- tap order, contraction, the weight total in double, the
passes swapped, mirrored borders, the window walked the other way -- changes
some float of some case at every scale, so the device comparison would see it.

The tally is a condition on the inputs, not a measurement of the device.
`python tests/test_scale_cases_cpu.py` prints it; profiles/scale_cases_tally.txt
keeps that output.  The tests recompute it and do not read the file."""
import os
import re

import numpy as np
import pytest

import scale_cases as sc  # tests/scale_cases.py
import scale_ref  # tests/scale_ref.py

SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                      "smvs_amd", "csrc", "scale.hip")

# (variant, scale) pairs at which the variant is the restatement itself, each
# found by measurement (the tally) and explained:
#   wsum_double at scale 2: the five weights' double sum rounds to the float
#   that the float sum reaches.
NO_EFFECT = {("wsum_double", 2)}


def _source():
    with open(SOURCE) as f:
        return f.read()


def test_mirror_constants_are_the_sources():
    src = _source()

    def constant(name):
        m = re.search(r"(?:constexpr int|#define)\s+%s\s*=?\s*(\d+)" % name, src)
        assert m, name
        return int(m.group(1))

    assert constant("BLUR_X_LDS_FROM") == sc.BLUR_X_LDS_FROM
    assert constant("BLUR_X_ROWS") == sc.BLUR_X_ROWS
    assert constant("BLUR_ROWS") == sc.BLUR_ROWS
    assert constant("FUSE_ROWS") == sc.FUSE_ROWS
    assert constant("FUSE_COLS") == sc.FUSE_COLS
    assert constant("GRAD_ROWS") == sc.GRAD_ROWS
    # 256 elements of a row per workgroup of the x pass, 256 threads everywhere
    assert "(w * c + %d) / %d" % (sc.BLOCK - 1, sc.BLOCK) in src
    assert "(e0 + %d) / C + ks <= w - 1" % (sc.BLOCK - 1) in src
    assert set(re.findall(r"__launch_bounds__\((\d+)\)", src)) == {str(sc.BLOCK)}
    # the predicates themselves, as the mirror restates them
    assert "e0 / C - ks >= 0 && (e0 + 255) / C + ks <= w - 1" in src
    assert "y0 - 1 - KS >= 0 && y0 + FUSE_ROWS + KS <= h - 1" in src
    # the half widths with a compile-time form, and those with a fused one
    assert tuple(int(k) for k in re.findall(r"case (\d+): launch_blur_ks<\1>", src)) \
        == sc.COMPILED_HALF_WIDTHS
    assert tuple(int(k) for k in re.findall(r"case (\d+): return launch_blur_gradients_ks<\1>", src)) \
        == sc.FUSED_HALF_WIDTHS
    assert "float k[%d];" % sc.MAX_TAPS in src and "ks + 1 <= %d" % sc.MAX_TAPS in src
    assert "n < ((size_t)1 << 20)" in src and sc.ASYNC_FROM == 1 << 20


def test_half_widths_and_forms():
    assert [sc.half_width(s) for s in range(11)] == [1, 2, 2, 4, 7, 12, 23, 45, 90, 178, 355]
    assert [sc.x_form(s) for s in sc.SCALES] == ["rows"] * 5 + ["lds", "lds", "runtime"]
    assert [sc.has_fused(s) for s in sc.SCALES] == [True] * 6 + [False, False]
    assert [sc.refused(s) for s in range(11)] == [False] * 8 + [True] * 3


def test_edge_sizes_are_the_ones_worked_out_by_hand():
    """The mirror's searches against the closed forms: w1 = 511 / C + ks + 1,
    h1 = 9 m + 9 + ks + 1 with m = ceil((ks + 1) / 9)."""
    table = {0: (171, 172, 512, 513), 1: (172, 173, 513, 514), 2: (172, 173, 513, 514),
             3: (174, 175, 515, 516), 4: (177, 178, 518, 519), 7: (215, 216, 556, 557)}
    for scale, (a3, b3, a1, b1) in table.items():
        ks = sc.half_width(scale)
        assert sc.first_interior_width(3, ks) == b3 == a3 + 1 == 511 // 3 + ks + 1
        assert sc.first_interior_width(1, ks) == b1 == a1 + 1 == 511 + ks + 1
    heights = {0: 20, 1: 21, 2: 21, 3: 23, 4: 26, 5: 40}
    for scale, h1 in heights.items():
        ks = sc.half_width(scale)
        m = -(-(ks + 1) // 9)
        assert sc.first_inner_height(ks) == h1 == 9 * m + 9 + ks + 1
    assert sc.lds_widths(1) == [255, 256, 257, 513]
    assert sc.lds_widths(3) == [85, 86, 171]


@pytest.mark.parametrize("scale", sc.SCALES)
def test_every_edge_is_hit(scale):
    ks = sc.half_width(scale)
    for c in sc.CHANNELS:
        got = sc.sizes(scale, c)
        wh = [(w, h) for w, h, _ in got]
        assert len(set(wh)) == len(wh)
        assert max(w for w, _ in wh) <= 560 and max(h for _, h in wh) <= 110
        assert all(h <= 12 for w, h in wh if w > 260)
        # small images, the converter's tail-only launch, the clamps meeting
        for size in sc.SMALL:
            assert size in wh
        if c == 1:
            assert {sc.converter(w * h)[0] for w, h in sc.SMALL} == {0, 1}
        assert any(w < ks and h < ks for w, h in wh) or ks <= 3
        # some column's taps clamp on both sides (no image is that narrow at half width 1)
        assert any(w <= 2 * ks - 1 for w, _ in wh) or ks == 1
        # the seams of the fused tiles and of the x pass's workgroups
        for w in (254, 255, 256, 257, 258):
            assert (w, 11) in wh
        for h in (9, 10, 11):
            assert (5, h) in wh
        # x pass: workgroup counts 1, 2, >= 3
        blocks = {min(sc.x_blocks(w, c), 3) for w, _ in wh}
        assert blocks == {1, 2, 3}, (c, blocks)
        if sc.x_form(scale) == "lds":
            elements = {w * c for w, _ in wh}
            want = {255, 256, 257, 513} if c == 1 else {255, 258, 513}
            assert want <= elements
            # a workgroup that begins past pixel 0; RGB: one that begins inside a pixel
            firsts = {sc.lds_x_first(c, b) for w, _ in wh for b in range(sc.x_blocks(w, c))}
            assert any(x > 0 for x, _ in firsts)
            assert c == 1 or any(ch != 0 for _, ch in firsts)
        else:
            # `interior` on either side: no interior workgroup one pixel below
            # w1, exactly workgroup 1 at w1, and rows that do not fill the
            # last group of BLUR_X_ROWS
            w1 = sc.first_interior_width(c, ks)
            assert (w1 - 1, 6) in wh and (w1, 6) in wh
            assert sc.x_interior_blocks(w1 - 1, c, ks) == []
            assert sc.x_interior_blocks(w1, c, ks) == [1]
            assert (sc.BLOCK - 1 + sc.BLOCK) // c + ks == w1 - 1      # met with equality
            assert 6 % sc.BLUR_X_ROWS != 0
        # y pass
        if sc.has_fused(scale):
            h1 = sc.first_inner_height(ks)
            assert (5, h1 - 1) in wh and (5, h1) in wh
            assert sc.fused_inner_tiles(h1 - 1, ks) == []
            tiles = sc.fused_inner_tiles(h1, ks)
            assert len(tiles) == 1
            assert tiles[0] * sc.FUSE_ROWS + sc.FUSE_ROWS + ks == h1 - 1   # met with equality
            assert {min(sc.fused_tiles(w, h)[1], 3) for w, h in wh} == {1, 2, 3}
        else:
            for h in (8, 9, 10, 2 * ks + 4, 2 * ks + 5):
                assert (5, h) in wh
            # row blocks of blur_y_kernel whose taps clamp at both ends, at the
            # top only and at the bottom only
            kinds = {sc.y_block_clamps(h, ks, b) for _, h in wh for b in range(sc.y_row_blocks(h))}
            assert {(True, True), (True, False), (False, True)} <= kinds
            assert {min(sc.y_row_blocks(h), 3) for _, h in wh} == {1, 2, 3}
            assert {min(sc.grad_blocks(w, h)[1], 3) for w, h in wh} == {1, 2, 3}
    # fused tile columns and gradient blocks 1, 2, >= 3 over both channel counts
    both = [(w, h) for c in sc.CHANNELS for w, h, _ in sc.sizes(scale, c)]
    assert {min(sc.fused_tiles(w, h)[0], 3) for w, h in both} == {1, 2, 3}
    assert {min(sc.grad_blocks(w, h)[0], 3) for w, h in both} == {1, 2, 3}


def test_contents():
    for c in sc.CHANNELS:
        imgs = sc.images(258, 11, c, "seam")
        assert tuple(imgs) == sc.CONTENTS
        for name, img in imgs.items():
            assert img.dtype == np.uint8 and img.shape == ((11, 258, 3) if c == 3 else (11, 258))
        assert (imgs["white"] == 255).all() and (imgs["grey128"] == 128).all()
        assert not imgs["zero"].any()
        assert set(np.unique(imgs["checker"])) == {0, 255}
        assert (imgs["checker"][:, 1:] != imgs["checker"][:, :-1]).all()
        assert (imgs["checker"][1:] != imgs["checker"][:-1]).all()
        for name, at in (("impulse_corner", (0, 0)), ("impulse_seam", (8, 253))):
            assert (imgs[name][at] == 255).all()
            assert np.count_nonzero(imgs[name]) == c
        if c == 3:
            ramp = imgs["ramp"].astype(int)
            assert not (ramp[..., 0] == ramp[..., 1]).all() and not (ramp[..., 1] == ramp[..., 2]).all()
        assert tuple(sc.images(172, 6, c, "edge")) == ("random",)


def _restated(scale, c, w, h, group, variant=None):
    _, stack = sc.stacked(w, h, c, group)
    return scale_ref.planes_batch(stack, scale, **({variant: True} if variant else {}))


def _oracle_planes(oracle, scale, c, w, h, group):
    names, stack = sc.stacked(w, h, c, group)
    planes = [oracle.scale_planes(img, scale) for img in stack]
    return np.stack([p[0] for p in planes]), np.stack([p[1] for p in planes])


@pytest.mark.parametrize("scale", sc.SCALES)
def test_restatement_equals_oracle(oracle, scale):
    """Bit patterns, not values: -0 is not +0 here."""
    for c in sc.CHANNELS:
        for w, h, group in sc.sizes(scale, c):
            names = sc.stacked(w, h, c, group)[0]
            want = _oracle_planes(oracle, scale, c, w, h, group)
            got = _restated(scale, c, w, h, group)
            for plane, a, b in zip(("gradient", "hessian"), got, want):
                d = sc.first_difference(a, b)
                assert d is None, "scale %d %dx%dx%d %s %s: %d floats differ, first at %r: %r / %r" % (
                    scale, w, h, c, names[d[1][0]], plane, d[0], d[1][1:], d[2], d[3])


def test_constant_images_leave_rounding_residue(oracle):
    """A constant image's gradients are sum(v k) / wsum rounded, not zero: the
    figures that make such images worth running (14 x 12 x 3, scale 2)."""
    for value in (255, 128):
        img = np.full((12, 14, 3), value, np.uint8)
        g, h = oracle.scale_planes(img, 2)
        assert np.count_nonzero(g) == 120, (value, np.count_nonzero(g))
        assert np.abs(g).max() < 1e-6
        for a, b in zip(scale_ref.planes(img, 2), (g, h)):
            assert sc.first_difference(a, b) is None
    g, h = oracle.scale_planes(np.zeros((12, 14, 3), np.uint8), 2)
    assert not scale_ref.bits(g).any() and not scale_ref.bits(h).any()     # +0 everywhere


def variant_counts(scale, variant):
    """Floats of the case list's planes that the variant changes."""
    n = 0
    for c in sc.CHANNELS:
        for w, h, group in sc.sizes(scale, c):
            for a, b in zip(_restated(scale, c, w, h, group, variant),
                            _restated(scale, c, w, h, group)):
                n += int(np.count_nonzero(scale_ref.bits(a) != scale_ref.bits(b)))
    return n


def total_floats(scale):
    return sum(5 * w * h * len(sc.stacked(w, h, c, group)[0])
               for c in sc.CHANNELS for w, h, group in sc.sizes(scale, c))


def tally_lines():
    lines = ["scale  ks  images  floats    " + "  ".join("%11s" % v for v in scale_ref.VARIANTS)]
    for scale in sc.SCALES:
        n_img = sum(len(sc.stacked(w, h, c, g)[0]) for c in sc.CHANNELS for w, h, g in sc.sizes(scale, c))
        lines.append("%5d  %2d  %6d  %8d  " % (scale, sc.half_width(scale), n_img, total_floats(scale))
                     + "  ".join("%11d" % variant_counts(scale, v) for v in scale_ref.VARIANTS))
    return lines


@pytest.mark.parametrize("variant", scale_ref.VARIANTS)
def test_every_variant_shows_at_every_scale(variant):
    for scale in sc.SCALES:
        n = variant_counts(scale, variant)
        if (variant, scale) in NO_EFFECT:
            assert n == 0, "no longer without effect: take (%s, %d) out of NO_EFFECT" % (variant, scale)
        else:
            assert n > 0, (variant, scale)


if __name__ == "__main__":
    print("\n".join(tally_lines()))
