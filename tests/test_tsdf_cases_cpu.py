"""What makes tests/test_gpu_tsdf_cases.py meaningful, checked without a GPU
and without the oracle: on the numpy restatements alone (tests/tsdf_ref.py,
tests/tsdf_sparse_ref.py) the cases of tests/tsdf_cases.py take every
inside/outside configuration of a cell and every number of crossing edges a
cube has, emit and withhold quads for every reason on every axis, leave steps
1-8 at every step and meet each of their comparisons with equality, read images
of 1 to 4 channels, put cells and quads across 1 to 8 bricks, and push both
scans across a tile.  And a restatement with one subtle mistake gives other
bits on them.

The tallies are conditions on the inputs, not measurements of the device.
`python tests/test_tsdf_cases_cpu.py` prints them; profiles/
tsdf_cases_tally.txt keeps that output.  The tests recompute them and do not
read the file.  The case that is cut needs the oracle and is tallied by the GPU
test's printout only; every condition here is stated on the uncut cases."""
import functools

import numpy as np
import pytest

import tsdf_cases as tc  # tests/tsdf_cases.py
import tsdf_ref  # tests/tsdf_ref.py
import tsdf_sparse_ref  # tests/tsdf_sparse_ref.py

UNCUT = tc.UNCUT_NAMES
ALL_CONFIGS = set(range(1, 255))
ALL_M = {tc.m_of_config(c) for c in ALL_CONFIGS}
f32 = np.float32


@functools.lru_cache(maxsize=None)
def _field_tally(name):
    c = tc.get(name)
    return tc.tally_field(c.cams, c.depths, *c.box, **c.kw)


@functools.lru_cache(maxsize=None)
def _surface_tally(name):
    return tc.tally_surface(tc.field_of(name)[0])


@functools.lru_cache(maxsize=None)
def _brick_tally(name):
    F, _, col = tc.field_of(name)
    return tc.tally_bricks(F, col, tc.get(name).box[2])


def _split(counts):
    """non-zero entries before and from the scan's first tile boundary"""
    return int((counts[:tc.SCAN_TILE] > 0).sum()), int((counts[tc.SCAN_TILE:] > 0).sum())


def tally_lines(names=UNCUT):
    lines = []
    for name in names:
        c = tc.get(name)
        origin, voxel, dims = c.box
        f, s, b = _field_tally(name), _surface_tally(name), _brick_tally(name)
        sizes = " ".join("%dx%dx%d" % (d.shape[1], d.shape[0], 1 if im.ndim == 2 else im.shape[2])
                         for d, im in zip(c.depths, c.images))
        lines.append("tally %-19s grid %dx%dx%d voxel %g trunc %g min_weight %d views %s" % (
            (name,) + tuple(dims) + (voxel, c.kw["trunc"], c.kw["min_weight"], sizes)))
        lines.append("      pairs    " + "  ".join(
            "[%s] %d" % (k, v) for k, v in zip(tc.LEAVE, f["leave"].sum(axis=0))))
        lines.append("      equal    " + "  ".join("%s: %d" % kv for kv in f["equal"].items())
                     + "   " + "  ".join("%s: %d" % kv for kv in f["pixel"].items()))
        lines.append("      voxels   " + "  ".join("%s: %d" % kv for kv in f["weight"].items()))
        lines.append("      cells    active %d  configurations %d of 254  m %s  sign change but "
                     "incomplete %d" % (s["active"], len(s["configs"]),
                                        " ".join("%d:%d" % kv for kv in sorted(s["m"].items())),
                                        s["incomplete_sign_change"]))
        for a in range(3):
            lines.append("      axis %d   " % a + "  ".join(
                "P %s: quads %d, none for %s" % (
                    ("outside", "inside")[o], s["quads"][a, o],
                    ", ".join("%s %d" % (r, n) for r, n in zip(tc.NO_QUAD, s["no_quad"][a, o])))
                for o in (0, 1)))
        lines.append("      mesh     vertices %d  faces %d  most faces on one edge %d  zero normals %d"
                     % (s["vertices"], s["faces"], s["max_faces_per_edge"], s["zero_normals"]))
        lines.append("      bricks   %d, seeds %d, allocated %d  corners in 1/2/4/8 bricks %s  quads "
                     "in 1/2/4 %s  halo NaN outside %d, not allocated %d  dense-only complete "
                     "cells %d" % (b["bricks"], b["seeds"], b["allocated"],
                                   "/".join(str(b["corner_span"][k]) for k in (1, 2, 4, 8)),
                                   "/".join(str(b["quad_span"][k]) for k in (1, 2, 4)),
                                   b["halo_outside"], b["halo_unallocated"],
                                   b["dense_only_complete"]))
        if name == "tiles":
            vertices, quads = tc.block_counts(tc.field_of(name)[0])
            lines.append("      scans    point blocks %d: with vertices %d + %d, with quads %d + %d "
                         "(before + from block %d)  allocated bricks %d: with vertices %d + %d, "
                         "with quads %d + %d" % (
                             (len(vertices),) + _split(vertices) + _split(quads) + (tc.SCAN_TILE,)
                             + (b["allocated"],) + _split(b["vertices_by_slot"])
                             + _split(b["quads_by_slot"])))
    configs = set().union(*(_surface_tally(n)["configs"] for n in tc.ROUGH_UNCUT))
    ms = set().union(*(_surface_tally(n)["m"] for n in tc.ROUGH_UNCUT))
    lines.append("rough, uncut together: configurations %d of 254  m %s  (a cube has %s)  zero "
                 "normals %d" % (len(configs), sorted(ms), sorted(ALL_M),
                                 sum(_surface_tally(n)["zero_normals"] for n in tc.ROUGH_UNCUT)))
    return lines


# (the first two x edges may change places unseen: the sum starts from 0 and
# float addition commutes; every other exchange shows)
EDGE_ORDERS = {"x": (0, 2, 1, 3), "y": (1, 0, 2, 3), "z": (3, 1, 2, 0)}
CHANNEL_MISTAKES = ("4-as-grey", "2-as-rgb")


def other_edge_order(name, axis):
    """tsdf_ref.surface of a case with the four edges of one axis in another
    order (tsdf_ref.EDGES replaced for the call) -> the mesh"""
    c = tc.get(name)
    F, W, col = tc.field_of(name)
    a = "xyz".index(axis)
    edges = list(tsdf_ref.EDGES)
    edges[4 * a:4 * a + 4] = [tsdf_ref.EDGES[4 * a + p] for p in EDGE_ORDERS[axis]]
    kept, tsdf_ref.EDGES = tsdf_ref.EDGES, edges
    try:
        return tsdf_ref.surface(F, W, col, c.box[0], c.box[1], len(c.cams))
    finally:
        tsdf_ref.EDGES = kept


def rows_with_other_bits(a, b):
    a, b = (np.ascontiguousarray(x).reshape(len(x), -1) for x in (a, b))
    return int((a.view(np.uint8) != b.view(np.uint8)).any(axis=1).sum())


def reversed_views_field(name):
    c = tc.get(name)
    origin, voxel, dims = c.box
    return tsdf_ref.field(c.cams[::-1], c.depths[::-1], c.images[::-1], origin, voxel, dims,
                          **c.kw)[0]


def misread_mesh(mistake):
    c = tc.get("channels")
    origin, voxel, dims = c.box
    return tsdf_ref.fuse(c.cams, c.depths, tc.misread_channels(c.images, mistake), origin, voxel,
                         dims, **c.kw)


def wrong_restatement_lines():
    lines = []
    for axis in "xyz":
        lines.append("vertices another order of the %s edges %s moves:  " % (axis, EDGE_ORDERS[axis])
                     + "  ".join("%s %d" % (n, rows_with_other_bits(
                         other_edge_order(n, axis)["xyz"], tc.restated(n)["xyz"]))
                         for n in tc.ROUGH_UNCUT))
    lines.append("voxels the reversed view list changes:  " + "  ".join(
        "%s %d" % (n, rows_with_other_bits(reversed_views_field(n).ravel(),
                                           tc.field_of(n)[0].ravel())) for n in tc.EXACT_NAMES))
    lines.append("vertices a wrong channel rule recolours:  " + "  ".join(
        "%s %d" % (m, rows_with_other_bits(misread_mesh(m)["rgb"], tc.restated("channels")["rgb"]))
        for m in CHANNEL_MISTAKES))
    return lines


def cut_case_lines():
    """the cut case, through the oracle's cut (only `python tests/
    test_tsdf_cases_cpu.py` calls this; the tests here need no oracle)"""
    from oracle import pyoracle
    lines = []
    for name in (n for n in tc.NAMES if n not in UNCUT):
        c = tc.get(name)
        maps = pyoracle.cut_depth_maps(c.cams, c.depths, c.normals)[0]
        origin, voxel, dims = c.box
        out = tsdf_ref.fuse(c.cams, maps, c.images, origin, voxel, dims, **c.kw)
        s = tc.tally_surface(out["tsdf"])
        lines.append("tally %-19s (cut by the oracle) pixels kept %s of %s  known voxels %d  active "
                     "cells %d  configurations %d  sign change but incomplete %d  vertices %d  "
                     "faces %d  zero normals %d" % (
                         name, [int((m != 0).sum()) for m in maps],
                         [int((d != 0).sum()) for d in c.depths],
                         int((~np.isnan(out["tsdf"])).sum()), s["active"], len(s["configs"]),
                         s["incomplete_sign_change"], s["vertices"], s["faces"],
                         s["zero_normals"]))
    return lines


def test_print_the_tallies():
    print()
    print("\n".join(tally_lines(tuple(n for n in UNCUT if n != "tiles"))))


# ---------------------------------------------------------------------- rough
def test_rough_cases_take_every_configuration_and_every_m():
    tallies = [_surface_tally(n) for n in tc.ROUGH_UNCUT]
    configs = set().union(*(t["configs"] for t in tallies))
    assert configs == ALL_CONFIGS, sorted(ALL_CONFIGS - configs)
    assert ALL_M == {3, 4, 5, 6, 7, 8, 9, 12}
    assert set().union(*(t["m"] for t in tallies)) == ALL_M
    assert all(t["incomplete_sign_change"] > 0 for t in tallies)
    assert max(t["max_faces_per_edge"] for t in tallies) == 4


def test_rough_cases_emit_and_withhold_quads_for_every_reason():
    quads = sum(_surface_tally(n)["quads"] for n in tc.ROUGH_UNCUT)
    none = sum(_surface_tally(n)["no_quad"] for n in tc.ROUGH_UNCUT)
    assert (quads > 0).all(), quads                      # every (axis, orientation)
    assert (none.sum(axis=1) > 0).all(), none            # every reason on every axis


def test_rough_cases_have_voxels_below_min_weight():
    below = {n: _field_tally(n)["weight"]["0<W<min_weight"] for n in tc.ROUGH_UNCUT}
    assert sum(below.values()) > 0, below
    for n in tc.ROUGH_UNCUT:
        assert (below[n] > 0) == (tc.get(n).kw["min_weight"] == 2), below


def test_the_rough_grids():
    dims = {tc.get(n).box[2] for n in tc.ROUGH_UNCUT}
    assert {tc.ODD, tc.WHOLE, tc.ONE_IN} <= dims
    assert all(n % b == 0 for n, b in zip(tc.WHOLE, tc.BRICK))
    assert all(n % b == 1 for n, b in zip(tc.ONE_IN, tc.BRICK))
    assert all(n % b > 1 for n, b in zip(tc.ODD, tc.BRICK))
    assert {len(tc.get(n).cams) for n in tc.ROUGH_UNCUT} == {3, 5}
    assert {tc.get(n).kw["min_weight"] for n in tc.ROUGH_UNCUT} == {1, 2}
    mixed = tc.get("rough-one-in-mixed")
    assert mixed.depths[2].shape == (71, 80) != mixed.depths[0].shape
    assert [n for n in tc.NAMES if tc.get(n).cut] == ["rough-odd-5v-cut"]
    assert [n for n in tc.NAMES if n not in UNCUT] == ["rough-odd-5v-cut"]


@pytest.mark.parametrize("axis", ["x", "y", "z"])
def test_another_edge_order_within_an_axis_gives_other_positions(axis):
    name = tc.ROUGH_UNCUT[0]
    want = tc.restated(name)
    got = other_edge_order(name, axis)
    changed = rows_with_other_bits(got["xyz"], want["xyz"])
    print("\nedge order %s %s: vertices with other bits %d of %d"
          % (axis, EDGE_ORDERS[axis], changed, len(want["xyz"])))
    assert changed > 0
    assert np.array_equal(got["faces"], want["faces"])
    assert np.array_equal(tc.restated(name)["xyz"], tsdf_ref.surface(
        *tc.field_of(name), tc.get(name).box[0], tc.get(name).box[1],
        len(tc.get(name).cams))["xyz"])          # (the edge table is back in place)


# ---------------------------------------------------------------------- exact
@pytest.mark.parametrize("name", tc.EXACT_NAMES)
def test_exact_cases_leave_at_every_step_and_meet_every_equality(name):
    t = _field_tally(name)
    leave = t["leave"].sum(axis=0)
    assert (leave > 0).all(), dict(zip(tc.LEAVE, leave))
    assert all(v > 0 for v in t["equal"].values()), t["equal"]
    assert all(v > 0 for v in t["pixel"].values()), t["pixel"]
    # one voxel beyond the last column and row: counted by the step-4 leaves
    assert t["weight"]["F==0"] > 0


@pytest.mark.parametrize("name", tc.EXACT_NAMES)
def test_exact_inputs_are_exact(name):
    """R = I and dyadic intrinsics, origin, voxel size and truncation: proj, u and
    v of the voxel centres carry no rounding (they equal the double values)."""
    c = tc.get(name)
    origin, voxel, dims = c.box
    centres = [np.float64(origin[a]) + (np.arange(dims[a]) + 0.5) * voxel for a in range(3)]
    for a in range(3):
        assert np.array_equal(tsdf_ref._centres(origin, f32(voxel), dims[a], a), centres[a])
    for cam, d in zip(c.cams, c.depths):
        h, w = d.shape
        V = tsdf_ref.camera(cam, w, h)
        K = np.array([[8.0, 0, w / 2], [0, 8.0, h / 2], [0, 0, 1]])
        assert np.array_equal(np.float64(V["KR"]).reshape(3, 3), K)
        assert np.array_equal(np.float64(V["t"]), K @ cam.center)


@pytest.mark.parametrize("name", tc.EXACT_NAMES)
def test_a_zero_field_value_lies_in_an_active_cell_and_counts_as_outside(name):
    c = tc.get(name)
    F, W, _ = tc.field_of(name)
    k, j, i = tc.exact_f0_voxel(c)
    assert F[k, j, i] == 0 and W[k, j, i] == 3
    _, _, inside, active = tc._cells(F)
    cells = [(k - dk, j - dj, i - di) for dk in (0, 1) for dj in (0, 1) for di in (0, 1)]
    holding = [cell for cell in cells if active[cell]]
    assert holding, "no active cell has the zero voxel as a corner"
    for n, (dk, dj, di) in enumerate((dk, dj, di) for dk in (0, 1) for dj in (0, 1)
                                     for di in (0, 1)):
        if active[cells[n]]:
            assert not inside[cells[n]][di + 2 * dj + 4 * dk]
    # an edge from it to an inside neighbour crosses at t = 0 / (0 - Fb) = 0
    near = [F[k + 1, j, i], F[k - 1, j, i], F[k, j + 1, i], F[k, j - 1, i], F[k, j, i + 1],
            F[k, j, i - 1]]
    assert any(x < 0 for x in near), near


def test_the_shifted_exact_case_puts_the_same_voxels_on_brick_faces():
    a, b = tc.get("exact"), tc.get("exact-shifted")
    assert all(np.array_equal(x, y) for x, y in zip(a.depths, b.depths))
    Fa, Fb = tc.field_of("exact")[0], tc.field_of("exact-shifted")[0]
    sx, sy, sz = tc.EXACT_SHIFT
    assert np.array_equal(Fb[sz:, sy:, sx:], Fa, equal_nan=True)
    k, j, i = tc.exact_f0_voxel(b)
    assert i % tc.BRICK[0] == 0 and j % tc.BRICK[1] == tc.BRICK[1] - 1
    assert tsdf_sparse_ref.brick_dims(b.box[2]) == (2, 2, 2)
    t = _brick_tally("exact-shifted")
    assert t["corner_span"][2] > 0 and t["corner_span"][4] > 0 and t["quad_span"][2] > 0


@pytest.mark.parametrize("name", tc.EXACT_NAMES)
def test_the_order_of_the_views_shows_in_the_sum(name):
    want = tc.field_of(name)[0]
    got = reversed_views_field(name)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    changed = rows_with_other_bits(got.ravel(), want.ravel())
    print("\nviews reversed: voxels with other bits %d" % changed)
    assert changed > 0


# ------------------------------------------------------------------- channels
def test_channels_case_reads_one_to_four_channels():
    c = tc.get("channels")
    assert [1 if im.ndim == 2 else im.shape[2] for im in c.images] == [1, 2, 3, 4]
    t = _field_tally("channels")
    assert (t["leave"][:, 8] > 1000).all(), t["leave"]      # every view colours voxels


@pytest.mark.parametrize("mistake", CHANNEL_MISTAKES)
def test_a_wrong_channel_rule_gives_other_colours(mistake):
    want = tc.restated("channels")
    got = misread_mesh(mistake)
    for k in ("tsdf", "xyz", "faces"):
        assert np.array_equal(got[k], want[k], equal_nan=True)
    changed = rows_with_other_bits(got["rgb"], want["rgb"])
    print("\n%s: vertices with another colour %d of %d" % (mistake, changed, len(want["rgb"])))
    assert changed > 100


# --------------------------------------------------------------------- bricks
def test_cells_and_quads_span_every_number_of_bricks():
    names = tc.ROUGH_UNCUT
    corner = {k: sum(_brick_tally(n)["corner_span"][k] for n in names) for k in (1, 2, 4, 8)}
    quad = {k: sum(_brick_tally(n)["quad_span"][k] for n in names) for k in (1, 2, 4)}
    assert all(v > 0 for v in corner.values()), corner
    assert all(v > 0 for v in quad.values()), quad
    assert sum(_brick_tally(n)["halo_outside"] for n in names) > 0
    assert sum(_brick_tally(n)["halo_unallocated"] for n in names) > 0
    deep = _brick_tally("rough-deep-3v")
    assert deep["dense_only_complete"] > 0 and deep["halo_unallocated"] > 0
    assert 0 < deep["seeds"] < deep["allocated"] < deep["bricks"]


@pytest.mark.parametrize("name", [n for n in UNCUT if n != "tiles"])
def test_sparse_restatement_gives_the_dense_mesh_in_another_order(name):
    """the two restatements against each other on these inputs, before the
    device is judged against either"""
    dense, sparse = tc.restated(name), tc.restated(name, sparse=True)
    p = np.argsort(sparse["cells"], kind="stable")
    for k in ("xyz", "normals", "rgb", "confidence"):
        assert np.array_equal(sparse[k][p], dense[k]), k
    assert len(sparse["faces"]) == len(dense["faces"])


# ---------------------------------------------------------------------- tiles
def test_tiles_case_crosses_a_tile_in_both_scans():
    c = tc.get("tiles")
    F, _, col = tc.field_of("tiles")
    print()
    print("\n".join(tally_lines(("tiles",))[:-1]))
    vertices, quads = tc.block_counts(F)
    assert len(vertices) == -(-F.size // tc.POINT_BLOCK) > tc.SCAN_TILE
    assert min(_split(vertices) + _split(quads)) > 0
    stats = tc.restated("tiles", sparse=True)["stats"]
    assert stats["allocated_bricks"] > tc.SCAN_TILE
    b = _brick_tally("tiles")
    assert b["allocated"] == stats["allocated_bricks"] < stats["bricks"]
    assert min(_split(b["vertices_by_slot"]) + _split(b["quads_by_slot"])) > 0
    assert all(b["corner_span"][k] > 0 for k in (1, 2, 4, 8))
    assert all(b["quad_span"][k] > 0 for k in (1, 2, 4))
    assert b["halo_outside"] > 0 and b["halo_unallocated"] > 0 and b["dense_only_complete"] > 0
    assert len(c.cams) == 3


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print("\n".join(tally_lines() + cut_case_lines() + wrong_restatement_lines()))
