"""What makes tests/test_gpu_cut_cases.py meaningful, checked without a GPU:
the numpy restatement tests/cut_ref.py and the oracle's orc_cut_depth_maps
agree to the bit on every case of tests/cut_cases.py (two readings of
mesh_generator.cc pinned against each other before the device is judged), and
the cases really take every branch: each outcome of a (pixel, view) pair and
each final reason often enough, thresholds met so closely that a comparison in
float would decide differently, quotients in (-1, 0) that truncate into column
or row 0, and a projection with proj[2] == 0.

The tallies are conditions on the inputs, not measurements of the device.
`python tests/test_cut_cases_cpu.py` prints them; profiles/cut_cases_tally.txt
keeps that output.  The tests recompute them and do not read the file."""
import numpy as np
import pytest

import cut_cases as cc  # tests/cut_cases.py
import cut_ref  # tests/cut_ref.py

PAIR_FLOOR = 100          # per outcome and per final reason, over the case list
SENSITIVE_FLOOR = 20      # per threshold, over the two ladders
TRUNCATED_FLOOR = 100
THRESHOLDS = ("1.01", "0.997", "0.5", "2.0")


def outcome_counts(infos):
    """Pairs per outcome that the walk really visits (not after a `break`)."""
    n = np.zeros(len(cut_ref.OUTCOMES), np.int64)
    for info in infos:
        live = info["outcome_px"][~info["stopped_px"]]
        n += np.bincount(live, minlength=len(n))
    return n


def reason_counts(infos):
    n = np.zeros(len(cut_ref.REASONS), np.int64)
    for info in infos:
        n += np.bincount(info["reason"].ravel(), minlength=len(n))
    return n


def truncated_pairs(infos):
    """Accepted pairs (the projection lands inside view j) whose x or y
    quotient lies in (-1, 0): (int) sends it to column or row 0, floor to -1."""
    n = 0
    for info in infos:
        accepted = ~info["stopped_px"] & (info["outcome_px"] >= cut_ref.HOLE)
        with np.errstate(invalid="ignore"):
            q = info["quot"]
            between = ((q > -1) & (q < 0)).any(axis=-1)
        n += int((accepted & between).sum())
    return n


def float_sensitive_pairs(infos):
    """Per threshold: the visited pairs whose outcome changes when that
    comparison alone is evaluated in float32 instead of float64, on the
    restatement's own proj[2] and powers."""
    n = dict.fromkeys(THRESHOLDS, 0)
    for info in infos:
        ys, xs = info["pixels"]
        power = info["power"][ys, xs]
        for j in range(info["outcome_px"].shape[0]):
            got = ~np.isnan(info["dm_j"][j]) & ~info["stopped_px"][j]
            args = (info["dm_j"][j][got], info["proj"][j][got, 2], power[got],
                    info["power_j"][j][got], info["power_jj"][j][got])
            wide = cut_ref.compare(*args, dtype=np.float64)
            flt = cut_ref.compare(*args, dtype=np.float32)
            want = cut_ref.classify(*wide)
            assert np.array_equal(want, info["outcome_px"][j][got])
            for name, swap in zip(THRESHOLDS, ((0,), (1,), (2,), (3, 4))):
                mixed = [flt[k] if k in swap else wide[k] for k in range(5)]
                n[name] += int((cut_ref.classify(*mixed) != want).sum())
    return n


def tally_lines():
    lines = []
    total_o = np.zeros(len(cut_ref.OUTCOMES), np.int64)
    total_r = np.zeros(len(cut_ref.REASONS), np.int64)
    total_t = 0
    for name in cc.NAMES:
        infos = cc.restated(name)[2]
        o, r, t = outcome_counts(infos), reason_counts(infos), truncated_pairs(infos)
        total_o += o
        total_r += r
        total_t += t
        sizes = " ".join("%dx%d" % (d.shape[1], d.shape[0]) for d in cc.get(name).depths)
        lines.append("tally %-20s views %s" % (name, sizes))
        lines.append("      pairs   " + "  ".join(
            "%s %d" % (k, v) for k, v in list(zip(cut_ref.OUTCOMES, o))[1:]))
        lines.append("      pixels  " + "  ".join(
            "%s %d" % (k, v) for k, v in zip(cut_ref.REASONS, r))
            + "   quotient in (-1, 0) accepted %d" % t)
    lines.append("total pairs   " + "  ".join(
        "%s %d" % (k, v) for k, v in list(zip(cut_ref.OUTCOMES, total_o))[1:]))
    lines.append("total pixels  " + "  ".join(
        "%s %d" % (k, v) for k, v in zip(cut_ref.REASONS, total_r))
        + "   quotient in (-1, 0) accepted %d" % total_t)
    for name in ("threshold_ladder", "power_ladder"):
        s = float_sensitive_pairs(cc.restated(name)[2])
        lines.append("float-sensitive pairs %-17s " % name + "  ".join(
            "%s: %d" % (k, s[k]) for k in THRESHOLDS))
    for variant, _ in WRONG_KERNELS:
        lines.append("pixels a wrong kernel flips: %-15s " % variant + "  ".join(
            "%s %d" % (name, flipped_pixels(name, variant)) for name in cc.NAMES))
    return lines


@pytest.mark.parametrize("name", cc.NAMES)
def test_restatement_equals_oracle(oracle, name):
    want_d, want_n = cc.oracle_cut(oracle, name)
    got_d, got_n, infos = cc.restated(name)
    for i, (a, b) in enumerate(zip(got_n, want_n)):
        assert np.array_equal(a, b, equal_nan=True), "world normals of view %d" % i
    for i, (a, b) in enumerate(zip(got_d, want_d)):
        bad = np.argwhere(a != b)
        assert len(bad) == 0, "view %d pixel (x %d, y %d): restatement %r oracle %r; %s" % (
            i, bad[0][1], bad[0][0], a[tuple(bad[0])], b[tuple(bad[0])],
            cut_ref.describe(infos[i], *bad[0]))
        # the reason says the same as the map
        kept = infos[i]["reason"] == cut_ref.KEPT
        assert np.array_equal(kept, a != 0)
        assert np.array_equal(a[kept], cc.get(name).depths[i][kept])


def test_every_outcome_and_every_reason_occurs():
    print()
    print("\n".join(tally_lines()))
    mixed = outcome_counts(cc.restated("mixed_wide")[2])
    assert (mixed[1:] > 0).all(), dict(zip(cut_ref.OUTCOMES, mixed))
    o = sum(outcome_counts(cc.restated(n)[2]) for n in cc.NAMES)
    r = sum(reason_counts(cc.restated(n)[2]) for n in cc.NAMES)
    assert (o[1:] >= PAIR_FLOOR).all(), dict(zip(cut_ref.OUTCOMES, o))
    assert (r[1:] >= PAIR_FLOOR).all(), dict(zip(cut_ref.REASONS, r))
    assert sum(truncated_pairs(cc.restated(n)[2]) for n in cc.NAMES) >= TRUNCATED_FLOOR
    # the reversed list walks other pairs: the break stops other views
    a = outcome_counts(cc.restated("mixed_wide")[2])
    b = outcome_counts(cc.restated("mixed_wide_reversed")[2])
    assert not np.array_equal(a, b)


def test_the_ladders_meet_their_thresholds_within_float_rounding():
    n = dict.fromkeys(THRESHOLDS, 0)
    for name in ("threshold_ladder", "power_ladder"):
        for k, v in float_sensitive_pairs(cc.restated(name)[2]).items():
            n[k] += v
    assert all(v >= SENSITIVE_FLOOR for v in n.values()), n
    # and both sides of every threshold are taken on the ladders themselves
    t = outcome_counts(cc.restated("threshold_ladder")[2])
    p = outcome_counts(cc.restated("power_ladder")[2])
    for counts, kinds in ((t, (cut_ref.OCCLUDED, cut_ref.ADD, cut_ref.FRONT_SUB)),
                          (p, (cut_ref.BREAK, cut_ref.ADD, cut_ref.FRONT_SUB,
                               cut_ref.FRONT_IGNORED))):
        assert all(counts[k] >= PAIR_FLOOR for k in kinds), counts


# (variant of cut_ref.cut, the cases that must show it)
WRONG_KERNELS = (("float_compare", ("threshold_ladder", "power_ladder")),
                 ("floorf", ("mixed_wide", "backfacing", "behind_camera", "degenerate_sizes")),
                 ("no_behind_test", ("behind_camera",)))


def flipped_pixels(name, variant):
    """Pixels of a case whose cut map a kernel with that mistake gets wrong."""
    c = cc.get(name)
    wrong = cut_ref.cut(c.cams, c.depths, c.normals, variant=variant)[0]
    return sum(int((a != b).sum()) for a, b in zip(wrong, cc.restated(name)[0]))


@pytest.mark.parametrize("variant,names", WRONG_KERNELS, ids=[v for v, _ in WRONG_KERNELS])
def test_a_subtly_wrong_kernel_would_be_caught(variant, names):
    """By the restatement's count: each mistake changes the cut map of at
    least 50 pixels in every case named for it (no kernel is run)."""
    counts = {name: flipped_pixels(name, variant) for name in names}
    print("\nwrong-kernel %s: pixels that flip %s" % (variant, counts))
    assert all(v >= 50 for v in counts.values()), counts


def test_backfacing_pixels_are_cut_walked_and_still_seen():
    c = cc.get("backfacing")
    cut_d, _, infos = cc.restated("backfacing")
    block = np.zeros(c.depths[0].shape, bool)
    block[cc.BACKFACING_BLOCK] = True
    assert np.array_equal(infos[0]["reason"] == cut_ref.BACKFACING, block)
    assert block.sum() >= PAIR_FLOOR and not cut_d[0][block].any()
    # walked for nothing: their pairs have outcomes like anybody's
    assert (infos[0]["outcome"][1:, block] != cut_ref.NONE).all()
    # and the other views still find them: pixels of views 1 and 2 whose
    # projection lands in the block get past the hole test
    view0 = infos[0]["view"]
    for i in (1, 2):
        ys, xs = infos[i]["pixels"]
        q = infos[i]["quot"][0]
        with np.errstate(invalid="ignore"):
            inside = (q[:, 0] >= 0) & (q[:, 0] < view0.w) & (q[:, 1] >= 0) & (q[:, 1] < view0.h)
        hit = np.zeros(len(ys), bool)
        hit[inside] = block[q[inside, 1].astype(int), q[inside, 0].astype(int)]
        assert hit.sum() >= PAIR_FLOOR
        assert (infos[i]["outcome_px"][0][hit] > cut_ref.HOLE).all()


def test_principal_plane_pairs_have_a_zero_proj2_and_are_skipped():
    cut_d, _, infos = cc.restated("principal_plane")
    ys, xs = infos[0]["pixels"]
    for j, (x, y) in zip((1, 2), cc.PLANE_PIXELS):
        at = np.nonzero((ys == y) & (xs == x))[0]
        assert len(at) == 1
        proj = infos[0]["proj"][j, at[0]]
        assert proj[2] == 0
        assert (proj[0] == 0 and proj[1] == 0) if j == 1 else proj[0] != 0
        assert infos[0]["outcome"][j, y, x] == cut_ref.OUTSIDE
        # the ring view keeps the pixel, so a pair that were not skipped shows
        assert infos[0]["reason"][y, x] == cut_ref.KEPT and cut_d[0][y, x] != 0
    # pixel (0, 0) of view 1 is what a NaN -> 0 conversion would read: it has a
    # depth, and its power, subtracted, would outweigh what the ring view adds
    c = cc.get("principal_plane")
    assert c.depths[1][0, 0] > 0
    view1 = infos[1]["view"]
    x, y = cc.PLANE_PIXELS[0]
    normal = cc.restated("principal_plane")[1][1][0:1, 0]
    pos_j = view1.world_point(np.array([0]), np.array([0]), c.depths[1][0:1, 0])
    assert view1.surface_power(pos_j, normal)[0] > 10 * infos[0]["sum"][y, x] > 0


def test_the_case_list():
    assert len(cc.NAMES) == len(set(cc.NAMES)) == 8
    mixed = cc.get("mixed_wide")
    assert [d.shape for d in mixed.depths] == [(63, 97), (97, 63), (121, 161), (30, 40),
                                               (47, 33), (63, 97)]
    assert len({c.flen for c in mixed.cams}) == 4
    assert [im.ndim for im in mixed.images] == [3, 2, 3, 2, 3, 2]
    rev = cc.get("mixed_wide_reversed")
    assert all(np.array_equal(a, b) for a, b in zip(rev.depths, mixed.depths[::-1]))
    deg = cc.get("degenerate_sizes")
    assert [d.shape for d in deg.depths] == [(63, 97), (2, 2), (30, 40), (300, 1), (63, 97)]
    assert not deg.depths[2].any()
    for name in cc.NAMES:
        c = cc.get(name)
        assert len(c.cams) == len(c.depths) == len(c.normals) == len(c.images)
        for d, n, im in zip(c.depths, c.normals, c.images):
            assert d.dtype == np.float32 and n.shape == d.shape + (3,)
            assert im.dtype == np.uint8 and im.shape[:2] == d.shape
            assert max(d.shape) <= 300 and d.size <= 161 * 121
    for name in ("threshold_ladder", "power_ladder"):
        a = cc.get(name).cams[0]
        for b in cc.get(name).cams[1:]:
            assert np.array_equal(a.R, b.R) and np.array_equal(a.t, b.t)


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print("\n".join(tally_lines()))
