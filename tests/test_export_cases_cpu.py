"""What makes tests/test_gpu_export_cases.py meaningful, checked without a GPU:
on the inputs of tests/export_cases.py the decisive events of every rule of
DESIGN.md section 9 occur often enough (the floors), and a restatement that
gets one rule wrong -- the `variant` argument of tests/points_reference.cc and
tests/simplify_reference.cc -- computes something else on at least one named
run, so that a kernel with that mistake could not pass the device comparison.

The floors are conditions on the inputs, not measurements of the device.
`python tests/test_export_cases_cpu.py` prints the tally and writes it to
profiles/export_cases_tally.txt; the tests recompute it and do not read the
file."""
import numpy as np
import pytest

import export_cases as ec  # tests/export_cases.py
import points_ref  # tests/points_ref.py
import simplify_ref  # tests/simplify_ref.py
from points_ref import (STAT_AXIS, STAT_DIAG, STAT_DISC, STAT_EDGES, STAT_EQUAL, STAT_MASK,
                        STAT_TIES, VERTEX_CLASS)
from simplify_ref import (SSTAT_FIVE, SSTAT_FOUR, SSTAT_NEAR, SSTAT_NOOP, SSTAT_OTHER,
                          SSTAT_RATIO, SSTAT_ROWS, SSTAT_TIED_SCANS, SSTAT_TIED_TOPS,
                          SSTAT_VALID, SSTAT_ZERO)

COMPLEX_FLOOR = 50             # regular grid
COMPLEX_SIMPLIFIED_FLOOR = 10
TIE_FLOOR = 200                # P2
MASK_FLOOR = 5
EDGE_FLOOR = 20                # per P3 threshold side, edge direction and dd_factor
RING_FLOOR = 20                # per confidence value
S10_FLOOR = 20                 # per clause
ROWS_FLOOR = 4000
RINGS = (0.0, 0.25, 0.5, 0.75, 1.0)

PLAIN_RUNS = tuple(r for r in ec.UNCUT_RUNS if not r.aabb)
PLAIN_SIMPLIFY_RUNS = tuple(r for r in ec.SIMPLIFY_RUNS if not r.aabb)
LADDER_RUNS = {r.dd_factor: r for r in ec.REGULAR_RUNS if r.case == "disc_ladder"}
BY_ID = {r.id: r for r in ec.REGULAR_RUNS + ec.SIMPLIFY_RUNS}

# the rules of points_reference.cc, on the regular grid and (P8-P10) on the
# simplified mesh; those of simplify_reference.cc
POINT_VARIANTS = ("P2_tie_le", "P3_ge", "P3_footprint_max", "P3_no_sqrt2", "P8_prepend_first",
                  "P9_unsorted", "P10_complex_seeds")
SIMPLIFY_VARIANTS = ("S6_latest", "S7_ge", "S8_multiply", "S10_ge4", "S10_own_triangle",
                     "S3_no_fallback")
# variant -> a run that must show it (the tally lists every run that does)
CAUGHT_BY = {"P2_tie_le": "quantised", "P3_ge": "disc_ladder-dd5",
             "P3_footprint_max": "disc_ladder-dd20", "P3_no_sqrt2": "disc_ladder-dd0.5",
             "P8_prepend_first": "holes_dense", "P9_unsorted": "holes_dense",
             "P10_complex_seeds": "rings", "S6_latest": "terraces", "S7_ge": "terraces",
             "S8_multiply": "terraces", "S10_ge4": "hole_blocks",
             "S10_own_triangle": "hole_blocks", "S3_no_fallback": "hole_blocks"}


def _face_counts(p):
    return np.bincount(p["faces"].ravel().astype(np.int64), minlength=len(p["xyz"]))


def regular_tally():
    """Per plain regular run: classes, masks, ties, P3 sides, rings, faces per
    vertex."""
    rows = {}
    for run in PLAIN_RUNS:
        p = ec.restated_points(run)
        st = p["stats"]
        rows[run.id] = dict(
            vertices=len(p["xyz"]), faces=len(p["faces"]),
            classes=np.bincount(p["vclass"], minlength=4),
            masks=st[STAT_MASK:STAT_MASK + 16], ties=int(st[STAT_TIES]),
            edges=int(st[STAT_EDGES]), disc=int(st[STAT_DISC]),
            axis=st[STAT_AXIS:STAT_AXIS + 3], diag=st[STAT_DIAG:STAT_DIAG + 3],
            equal=int(st[STAT_EQUAL]),
            rings=np.array([(p["confidence"] == F).sum() for F in np.float32(RINGS)]),
            degree=np.bincount(_face_counts(p), minlength=9))
    return rows


def simplify_tally():
    rows = {}
    for run in PLAIN_SIMPLIFY_RUNS:
        s = ec.restated_simplified(run, False)
        rows[run.id] = dict(vertices=len(s["xyz"]), faces=len(s["faces"]), stats=s["stats"],
                            classes=np.bincount(s["vclass"], minlength=4))
    return rows


def _rows_differing(a, b, keys):
    """Rows that differ in any of the keys, plus the difference in length."""
    n = min(len(a[keys[0]]), len(b[keys[0]]))
    bad = np.zeros(n, bool)
    for k in keys if n else ():
        x, y = a[k][:n].reshape(n, -1), b[k][:n].reshape(n, -1)
        bad |= ~((x == y) | ((x != x) & (y != y))).all(axis=1)
    return int(bad.sum()) + abs(len(a[keys[0]]) - len(b[keys[0]]))


def changed_by(variant, run):
    """(vertices, faces) of a run that the variant changes in the exported
    point cloud; for the simplified runs the raw triangulations count too."""
    if isinstance(run, ec.Run):
        want, got = ec.restated_points(run), ec.restated_points(run, variant)
    else:
        want, got = ec.restated_simplified(run, False), ec.restated_simplified(run, False, variant)
    v = _rows_differing(got, want, ("xyz", "normals", "rgb", "confidence", "value"))
    f = _rows_differing(got, want, ("faces",))
    if isinstance(run, ec.SimplifyRun):
        for view in range(len(ec.get(run.case).depths)):
            a = ec.restated_triangulation(run, view)
            b = ec.restated_triangulation(run, view, variant)
            v += _rows_differing(b, a, ("vertices",))
            f += _rows_differing(b, a, ("triangles",)) + _rows_differing(b, a, ("num_zero_depths",))
            f += int(a["iterations"] != b["iterations"])
    return v, f


@pytest.fixture(scope="module")
def variant_table():
    return variant_changes()


_VARIANT_CHANGES = {}


def variant_changes():
    """variant -> {run id: (vertices, faces) changed}, the runs that change."""
    if not _VARIANT_CHANGES:
        for variant in POINT_VARIANTS + SIMPLIFY_VARIANTS:
            runs = PLAIN_SIMPLIFY_RUNS if variant in SIMPLIFY_VARIANTS else PLAIN_RUNS
            if variant in ("P8_prepend_first", "P9_unsorted", "P10_complex_seeds"):
                runs = runs + PLAIN_SIMPLIFY_RUNS
            table = {}
            for run in runs:
                v, f = changed_by(variant, run)
                if v or f:
                    table[run.id] = (v, f)
            _VARIANT_CHANGES[variant] = table
    return _VARIANT_CHANGES


def tally_lines():
    lines = ["regular grid (points_ref on the uncut runs)"]
    reg = regular_tally()
    for rid, r in reg.items():
        lines.append("tally %-18s vertices %d faces %d  unref/simple/border/complex %s" % (
            rid, r["vertices"], r["faces"], " ".join(str(v) for v in r["classes"])))
        lines.append("      masks 0..15 %s" % " ".join(str(v) for v in r["masks"]))
        lines.append("      P2 ties %d  P3 edges %d discontinuities %d equal depths %d" % (
            r["ties"], r["edges"], r["disc"], r["equal"]))
        lines.append("      P3 last-below/at/first-above: axis %s diagonal %s" % (
            "/".join(str(v) for v in r["axis"]), "/".join(str(v) for v in r["diag"])))
        lines.append("      confidences 0,1/4,1/2,3/4,1: %s   vertices with 0..8 faces: %s" % (
            " ".join(str(v) for v in r["rings"]), " ".join(str(v) for v in r["degree"][:9])))
    lines.append("total complex %d  P2 ties %d  masks %s  rings %s" % (
        sum(r["classes"][3] for r in reg.values()), sum(r["ties"] for r in reg.values()),
        " ".join(str(v) for v in sum(r["masks"] for r in reg.values())),
        " ".join(str(v) for v in sum(r["rings"] for r in reg.values()))))
    lines.append("simplified (simplify_ref on every view of the runs)")
    sim = simplify_tally()
    for rid, r in sim.items():
        st = r["stats"]
        lines.append("tally %-24s vertices %d faces %d  unref/simple/border/complex %s" % (
            rid, r["vertices"], r["faces"], " ".join(str(v) for v in r["classes"])))
        lines.append("      S5 no-ops %d  S6 tied tops %d  S7 tied scans %d  tallest triangle %d rows"
                     % (st[SSTAT_NOOP], st[SSTAT_TIED_TOPS], st[SSTAT_TIED_SCANS], st[SSTAT_ROWS]))
        lines.append("      S10 removed: zero depths %d edge ratio %d;  k-th triangle has 4 / 5 "
                     "zeros %d / %d, is not the face's own %d;  ratio in [0.1, 0.2) %d" % (
                         st[SSTAT_ZERO], st[SSTAT_RATIO], st[SSTAT_FOUR], st[SSTAT_FIVE],
                         st[SSTAT_OTHER], st[SSTAT_NEAR]))
    total = sum(r["stats"] for r in sim.values())
    lines.append("total complex %d  S10 zero depths %d edge ratio %d  S6 tied tops %d  "
                 "S7 tied scans %d" % (sum(r["classes"][3] for r in sim.values()),
                                       total[SSTAT_ZERO], total[SSTAT_RATIO],
                                       total[SSTAT_TIED_TOPS], total[SSTAT_TIED_SCANS]))
    lines.append("what a restatement with one rule wrong changes: run (vertices, faces)")
    for variant, table in variant_changes().items():
        lines.append("variant %-18s %s" % (variant, "  ".join(
            "%s (%d, %d)" % (rid, v, f) for rid, (v, f) in table.items()) or "NOTHING"))
    return lines


# ------------------------------------------------------------------ floors
def test_regular_grid_floors():
    reg = regular_tally()
    print()
    print("\n".join(tally_lines()))
    assert sum(r["classes"][VERTEX_CLASS["complex"]] for r in reg.values()) >= COMPLEX_FLOOR
    assert sum(r["ties"] for r in reg.values()) >= TIE_FLOOR
    assert (sum(r["masks"] for r in reg.values()) >= MASK_FLOOR).all()
    assert (sum(r["rings"] for r in reg.values()) >= RING_FLOOR).all()
    # holes_dense: all 16 masks, every class in hundreds
    dense = reg["holes_dense"]
    assert (dense["masks"] >= MASK_FLOOR).all()
    assert (dense["classes"][1:] >= 100).all(), dense["classes"]
    # quantised: the diagonal choice alternates, 4- and 8-face vertices
    q = reg["quantised"]
    assert q["ties"] >= TIE_FLOOR and q["masks"][15] - q["ties"] >= TIE_FLOOR
    assert q["degree"][4] >= 20 and q["degree"][8] >= 20
    # rings: every ring value in one view, and the planted complex vertices
    # carry a ring value of their own (P10: not seeds)
    r = reg["rings"]
    assert (r["rings"] >= RING_FLOOR).all()
    assert r["classes"][VERTEX_CLASS["complex"]] == len(ec.RINGS_COMPLEX)
    p = ec.restated_points(BY_ID["rings"])
    assert (p["confidence"][p["vclass"] == VERTEX_CLASS["complex"]] > 0).all()


@pytest.mark.parametrize("factor", ec.DD_FACTORS[1:])
def test_ladder_straddles_the_threshold(factor):
    st = ec.restated_points(LADDER_RUNS[factor])["stats"]
    for name, at in (("axis", STAT_AXIS), ("diagonal", STAT_DIAG)):
        assert (st[at:at + 3] >= EDGE_FLOOR).all(), (name, st[at:at + 3])
    assert st[STAT_EQUAL] >= EDGE_FLOOR
    # both outcomes, and a factor changes them
    assert EDGE_FLOOR <= st[STAT_DISC] <= st[STAT_EDGES] - EDGE_FLOOR


def test_ladder_without_the_test_keeps_every_triangle():
    """dd_factor = 0 skips P3: one triangle per built block, two per block of
    equal depths, none dropped; every other factor drops some."""
    zero = ec.restated_points(LADDER_RUNS[0.0])
    assert zero["stats"][STAT_EDGES] == 0
    plan = ec.ladder_plan()
    assert len(zero["faces"]) == sum(2 if p[2] is None else 1 for p in plan)
    counts = [len(ec.restated_points(LADDER_RUNS[f])["faces"]) for f in ec.DD_FACTORS]
    assert counts[1] < counts[2] < counts[3] < counts[0], counts


def test_ladder_footprints_are_the_restatement_s():
    """export_cases.footprints (numpy) against pixel_footprint of
    points_reference.cc, on the ladder's own pixels and depths."""
    d = ec.get("disc_ladder").depths[0]
    ys, xs = np.nonzero(d)
    pick = np.arange(0, len(ys), 37)
    got = ec.footprints(ec.LADDER_W, ec.LADDER_H, ec.FLEN, xs[pick], ys[pick], d[ys[pick], xs[pick]])
    want = [points_ref.footprint(ec.LADDER_W, ec.LADDER_H, ec.FLEN, int(x), int(y), d[y, x])
            for x, y in zip(xs[pick], ys[pick])]
    assert len(pick) > 100 and np.array_equal(got, np.array(want, np.float32))


def test_simplified_floors():
    sim = simplify_tally()
    total = sum(r["stats"] for r in sim.values())
    assert total[SSTAT_ZERO] >= S10_FLOOR and total[SSTAT_RATIO] >= S10_FLOOR
    assert sum(r["classes"][VERTEX_CLASS["complex"]] for r in sim.values()) \
        >= COMPLEX_SIMPLIFIED_FLOOR
    assert total[SSTAT_TIED_TOPS] >= 20 and total[SSTAT_TIED_SCANS] >= 100
    # terraces: equal keys and equal distances decide (S6, S7)
    t = sim["terraces"]["stats"]
    assert t[SSTAT_TIED_TOPS] >= 10 and t[SSTAT_TIED_SCANS] >= 100
    # exhaustive: the loop runs into S5 by itself, on a map with depth
    e = sim["exhaustive"]["stats"]
    tri = ec.restated_triangulation(BY_ID["exhaustive"])
    budget = 24 * 16 + 10
    assert e[SSTAT_NOOP] >= 1 and e[SSTAT_VALID] == 1
    assert tri["iterations"] == budget > len(tri["vertices"]) - 4 > 300
    # hole_blocks: S10's `> 4` straddled, S11 busy, corners zero, complex after
    hb = sim["hole_blocks"]
    assert hb["stats"][SSTAT_FOUR] >= 5 and hb["stats"][SSTAT_FIVE] >= 5
    assert hb["stats"][SSTAT_ZERO] >= S10_FLOOR and hb["stats"][SSTAT_OTHER] >= 100
    assert hb["classes"][VERTEX_CLASS["complex"]] >= 5
    d = ec.get("hole_blocks").depths[0]
    assert d[0, 0] == d[0, -1] == d[-1, 0] == d[-1, -1] == 0
    # slivers: both sides of 0.1
    s = sim["slivers"]["stats"]
    assert s[SSTAT_RATIO] >= 10 and s[SSTAT_NEAR] >= 10


def test_limits():
    budgets = {}
    for w, h in ec.LIMIT_SIZES:
        run = BY_ID["limits_%dx%d" % (w, h)]
        d = ec.get(run.case).depths[0]
        assert d.shape == (h, w) and len(np.unique(d)) <= 3
        tri = ec.restated_triangulation(run)
        budgets[(w, h)] = simplify_ref.budget(w, h)
        assert tri["iterations"] == budgets[(w, h)]
    assert list(budgets.values()) == [204, 204, 0, 2, 22]
    # a triangle of 4098 rows (the LDS row table holds 4100), column 4096 + 1
    assert ec.restated_triangulation(BY_ID["limits_2x4096"])["stats"][SSTAT_ROWS] > ROWS_FLOOR
    wide = ec.restated_triangulation(BY_ID["limits_4096x2"])
    assert wide["vertices"][:, 0].max() == 4096
    assert (wide["vertices"][4:, 0] >= 2048).any()
    # budget 0: nothing is left after S9
    assert len(ec.restated_simplified(BY_ID["limits_2x2"], False)["xyz"]) == 0


# ---------------------------------------------------------------- variants
@pytest.mark.parametrize("variant", POINT_VARIANTS + SIMPLIFY_VARIANTS)
def test_a_restatement_with_one_rule_wrong_differs(variant_table, variant):
    table = variant_table[variant]
    print("\nvariant %s changes (vertices, faces): %s" % (variant, table))
    assert CAUGHT_BY[variant] in table, table


def test_variant_zero_is_the_pinned_behaviour():
    """The hand-checked pins of test_points_cpu.py and test_simplify_cpu.py,
    through the entries that now take a variant."""
    import test_points_cpu as tp
    for mask in range(16):
        tp.test_single_block_masks(mask)
    tp.test_four_valid_corners_split_along_smaller_depth_difference()
    tp.test_full_3x3_grid_eight_triangles_and_vertex_order()
    tp.test_depth_discontinuity_straight_edge()
    tp.test_depth_discontinuity_diagonal_edge()
    tp.test_blocks_touching_at_a_corner_make_a_complex_vertex()
    tp.test_confidence_rings_of_a_square()
    assert points_ref.VARIANTS[None] == 0
    assert sorted(points_ref.VARIANTS.values()) == list(range(len(points_ref.VARIANTS)))
    # and an explicit None is the default, to the bit
    run = BY_ID["holes_dense"]
    c = ec.get(run.case)
    dms, wn = ec.maps(run.case)
    again = points_ref.points(c.cams, dms, wn, c.images)
    want = ec.restated_points(run)
    for k in ("xyz", "normals", "rgb", "confidence", "value", "faces"):
        assert again[k].tobytes() == want[k].tobytes(), k
    zero = np.zeros((20, 30), np.float32)
    tri = simplify_ref.triangulate(zero)
    assert tri["iterations"] == 15 and len(tri["vertices"]) == 5


# ---------------------------------------------------------------- the list
def test_mixed_sizes_and_empty_views(oracle):
    mixed = ec.get("mixed_sizes")
    assert [d.shape[::-1] for d in mixed.depths] == [v[2:4] for v in ec.MIXED_VIEWS]
    assert [d.shape[::-1] for d in mixed.depths] == [(97, 63), (2, 2), (40, 30), (2, 57), (1, 50),
                                                      (63, 97), (161, 121)]
    assert sorted({im.ndim for im in mixed.images}) == [2, 3]
    dms, wn = ec.maps("mixed_sizes")
    parts = [points_ref.view(c, d, n, i) for c, d, n, i in zip(mixed.cams, dms, wn, mixed.images)]
    assert len(parts[ec.ONE_COLUMN_VIEW]["xyz"]) == 0 and mixed.depths[ec.ONE_COLUMN_VIEW].all()
    assert all(len(p["faces"]) > 0 for i, p in enumerate(parts) if i != ec.ONE_COLUMN_VIEW)
    # the cut removes pixels, differently in the reversed list
    cut = ec.restated_points(BY_ID["mixed_sizes-cut"], oracle=oracle)
    rev = ec.restated_points(BY_ID["mixed_sizes_reversed-cut"], oracle=oracle)
    plain = ec.restated_points(BY_ID["mixed_sizes"])
    assert 0 < len(cut["xyz"]) < len(plain["xyz"]) and 0 < len(rev["xyz"]) < len(plain["xyz"])
    assert not np.array_equal(rev["xyz"][:100], cut["xyz"][:100])
    # cut_ref's world normals are the oracle's
    for c, d, n, w in zip(mixed.cams, mixed.depths, mixed.normals, wn):
        assert np.array_equal(oracle.cut_depth_maps([c], [d], [n])[1][0], w)
    rev_case = ec.get("mixed_sizes_reversed")
    assert all(np.array_equal(a, b) for a, b in zip(rev_case.depths, mixed.depths[::-1]))
    # the simplified list: no one-column view, one view without depth
    simp = ec.get("mixed_sizes_simplified")
    assert min(min(d.shape) for d in simp.depths) == 2 and len(simp.depths) == len(mixed.depths) - 1
    assert not simp.depths[ec.EMPTIED_VIEW].any()
    holes = ec.get("all_holes_view")
    assert not holes.depths[1].any() and holes.depths[0].any() and holes.depths[2].any()


@pytest.mark.parametrize("rid", ["holes_dense-aabb", "mixed_sizes-aabb"])
def test_the_box_cuts_through_faces_in_every_view(rid):
    run = BY_ID[rid]
    c = ec.get(run.case)
    dms, wn = ec.maps(run.case)
    lo, hi = np.float32(ec.box(run))
    for cam, d, n, im in zip(c.cams, dms, wn, c.images):
        p = points_ref.view(cam, d, n, im)
        if len(p["faces"]) < 10:
            continue
        inside = ~((p["xyz"] < lo) | (p["xyz"] > hi)).any(axis=1)
        corners = inside[p["faces"]].sum(axis=1)
        assert (corners == 3).any() and ((corners > 0) & (corners < 3)).any(), d.shape
    clipped = ec.restated_mesh(run)
    assert 0 < len(clipped["faces"]) and np.all(clipped["normals"] == 0, axis=1).any()


def test_the_case_list():
    names = ec.REGULAR_NAMES + ec.SIMPLIFY_NAMES
    assert len(names) == len(set(names))
    assert {r.case for r in ec.REGULAR_RUNS} == set(ec.REGULAR_NAMES)
    assert {r.case for r in ec.SIMPLIFY_RUNS} == set(ec.SIMPLIFY_NAMES)
    assert sorted(LADDER_RUNS) == sorted(ec.DD_FACTORS)
    for name in names:
        c = ec.get(name)
        assert len(c.cams) == len(c.depths) == len(c.normals) == len(c.images)
        for d, n, im in zip(c.depths, c.normals, c.images):
            assert d.dtype == np.float32 and n.shape == d.shape + (3,)
            assert im.dtype == np.uint8 and im.shape[:2] == d.shape
            assert np.isfinite(d).all() and (d >= 0).all()
            if not name.startswith("limits_"):
                assert d.shape[1] <= 161 and d.shape[0] <= 121


DEVICE_SECTION = "measured on the device"


if __name__ == "__main__":
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    text = "\n".join(tally_lines()) + "\n"
    print(text, end="")
    # the section that test_gpu_export_cases.py's output was copied into stays
    path = os.path.join(root, "profiles", "export_cases_tally.txt")
    kept = ""
    if os.path.exists(path):
        with open(path) as f:
            old = f.read()
        if DEVICE_SECTION in old:
            kept = old[old.index(DEVICE_SECTION):]
    with open(path, "w") as f:
        f.write(text + kept)
