"""Known answers of the point export's semantics on
tiny maps, through the serial CPU restatement tests/points_reference.cc, and
the host PLY writer read back by an independent reader.  No GPU."""
import os
import types

import numpy as np
import pytest

import points_ref  # tests/points_ref.py

IDENT = types.SimpleNamespace(flen=1.0, R=np.eye(3, dtype=np.float32),
                              t=np.zeros(3, np.float32))


def _index_image(h, w):
    """Colour = pixel index (r + 256 g + 65536 b): the exported colours tell
    which pixel became which vertex."""
    i = np.arange(h * w, dtype=np.int64).reshape(h, w)
    return np.stack([i & 255, (i >> 8) & 255, (i >> 16) & 255], axis=-1).astype(np.uint8)


def _pixels(out):
    rgb = out["rgb"].astype(np.int64)
    return rgb[:, 0] + 256 * rgb[:, 1] + 65536 * rgb[:, 2]


def _run(dm, cam=IDENT, dd_factor=5.0):
    dm = np.asarray(dm, np.float32)
    h, w = dm.shape
    nrm = np.zeros((h, w, 3), np.float32)
    out = points_ref.view(cam, dm, nrm, _index_image(h, w), dd_factor)
    out["pixel"] = _pixels(out)
    return out


def _faces_as_pixels(out):
    return [tuple(int(out["pixel"][v]) for v in f) for f in out["faces"]]


# depthmap_triangulate's triangles per mask of one 2 x 2 block (corners
# 0 = (0,0), 1 = (1,0), 2 = (0,1), 3 = (1,1); 2 x 2 map: corner = pixel index)
MASK_FACES = {7: [(0, 2, 1)], 11: [(0, 3, 1)], 13: [(0, 2, 3)], 14: [(1, 2, 3)],
              15: [(0, 2, 1), (1, 2, 3)]}


@pytest.mark.parametrize("mask", range(16))
def test_single_block_masks(mask):
    dm = np.array([[1.0 if mask & 1 else 0.0, 1.0 if mask & 2 else 0.0],
                   [1.0 if mask & 4 else 0.0, 1.0 if mask & 8 else 0.0]], np.float32)
    out = _run(dm)
    want = MASK_FACES.get(mask, [])
    assert _faces_as_pixels(out) == want
    order = []
    for f in want:
        for p in f:
            if p not in order:
                order.append(p)
    assert list(out["pixel"]) == order


def test_four_valid_corners_split_along_smaller_depth_difference():
    out = _run([[1.0, 1.2], [1.4, 1.0]])      # |d0 - d3| = 0 < |d1 - d2|
    assert _faces_as_pixels(out) == [(0, 3, 1), (0, 2, 3)]
    assert list(out["pixel"]) == [0, 3, 1, 2]


def test_full_3x3_grid_eight_triangles_and_vertex_order():
    out = _run(np.full((3, 3), 2.0, np.float32))
    assert len(out["faces"]) == 8
    assert list(out["pixel"]) == [0, 3, 1, 4, 2, 5, 6, 7, 8]
    # every vertex on the 3 x 3 border except the centre
    cls = dict(zip(out["pixel"].tolist(), out["vclass"].tolist()))
    assert cls[4] == points_ref.VERTEX_CLASS["simple"]
    assert all(cls[p] == points_ref.VERTEX_CLASS["border"] for p in cls if p != 4)


def _footprint(x, y, d, flen, w, h):
    """pixel_footprint in float32, restated with numpy."""
    f = np.float32
    dim = f(max(w, h))
    ax = f(flen) * dim
    inv = [f(1) / ax, f(0), f(-f(w) * f(0.5)) / ax, f(0), f(1) / ax,
           f(-f(h) * f(0.5)) / ax, f(0), f(0), f(1)]
    p = (f(x) + f(0.5), f(y) + f(0.5), f(1))
    v = [f(f(f(f(0) + inv[3 * r] * p[0]) + inv[3 * r + 1] * p[1]) + inv[3 * r + 2] * p[2])
         for r in range(3)]
    n = np.sqrt(f(f(f(f(0) + v[0] * v[0]) + v[1] * v[1]) + v[2] * v[2]))
    return f(f(inv[0] * f(d)) / n)


def _straddle(d_min, limit):
    """The largest float32 d with d - d_min <= limit, and the next one."""
    f = np.float32
    d = f(d_min) + f(limit)
    while f(d - f(d_min)) > limit:
        d = np.nextafter(d, f(0))
    while f(np.nextafter(d, f(np.inf)) - f(d_min)) <= limit:
        d = np.nextafter(d, f(np.inf))
    return d, np.nextafter(d, f(np.inf))


def test_depth_discontinuity_straight_edge():
    # mask 7: triangle (0, 2, 1); d0 = d2 = 1, d1 varies: the straight edge
    # 0-1 decides (the diagonal 2-1 has the larger threshold)
    f = np.float32
    limit = f(_footprint(0, 0, 1.0, 1.0, 2, 2) * f(5.0))
    keep, drop = _straddle(1.0, limit)
    assert len(_run([[1.0, keep], [1.0, 0.0]])["faces"]) == 1
    assert len(_run([[1.0, drop], [1.0, 0.0]])["faces"]) == 0


def test_depth_discontinuity_diagonal_edge():
    # mask 11: triangle (0, 3, 1); d3 = 1, d1 = d0 + 1/2 of the gap; d0 < 1
    # varies, so the diagonal 0-3 (factor 5 sqrt 2) is the tightest edge
    f = np.float32
    dd = f(np.float64(5.0) * 1.41421356237309504880)

    def dropped(d0):
        d0 = f(d0)
        d1 = f(f(d0 + f(1.0)) * f(0.5))
        out = _run([[d0, d1], [0.0, 1.0]])
        return len(out["faces"]) == 0, d0

    # footprint(d0) grows with d0: search the flip point by bisection on floats
    lo, hi = f(0.05), f(0.9)
    assert dropped(lo)[0] and not dropped(hi)[0]
    while np.nextafter(lo, f(1)) < hi:
        mid = f((np.float64(lo) + np.float64(hi)) / 2)
        if mid <= lo or mid >= hi:
            mid = np.nextafter(lo, f(1))
        if dropped(mid)[0]:
            lo = mid
        else:
            hi = mid
    # at the flip the diagonal predicate of the restatement flips
    for d0, want in ((lo, True), (hi, False)):
        disc = f(f(1.0) - d0) > f(_footprint(0, 0, d0, 1.0, 2, 2) * dd)
        assert disc == want
        assert dropped(d0)[0] == want


def test_isolated_valid_pixel_is_not_exported():
    dm = np.zeros((4, 4), np.float32)
    dm[1, 2] = 1.0
    out = _run(dm)
    assert len(out["xyz"]) == 0 and len(out["faces"]) == 0


def test_blocks_touching_at_a_corner_make_a_complex_vertex():
    # blocks (0,0) at depth 1 and (1,1) at depth 5 share the centre (2.4, a
    # continuous step from either side); the blocks across hold one triangle
    # each, whose diagonal from 1 to 5 is a discontinuity
    dm = np.array([[1.0, 1.0, 0.0],
                   [1.0, 2.4, 5.0],
                   [0.0, 5.0, 5.0]], np.float32)
    out = _run(dm)
    assert _faces_as_pixels(out) == [(0, 3, 1), (1, 3, 4), (4, 7, 5), (5, 7, 8)]
    cls = dict(zip(out["pixel"].tolist(), out["vclass"].tolist()))
    assert cls[4] == points_ref.VERTEX_CLASS["complex"]
    assert all(cls[p] == points_ref.VERTEX_CLASS["border"] for p in cls if p != 4)


def test_confidence_rings_of_a_square():
    n = 12
    out = _run(np.full((n, n), 3.0, np.float32))
    assert len(out["xyz"]) == n * n
    y, x = np.divmod(out["pixel"], n)
    ring = np.minimum(np.minimum(x, y), np.minimum(n - 1 - x, n - 1 - y))
    want = np.minimum(ring, 4).astype(np.float32) / np.float32(4)
    assert np.array_equal(out["confidence"], want)
    assert set(out["confidence"].tolist()) == {0.0, 0.25, 0.5, 0.75, 1.0}


def test_scale_value_of_a_fronto_parallel_plane():
    w, h, z, flen = 16, 12, 4.0, 1.0
    xs, ys = np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5)
    ax = flen * max(w, h)
    rx, ry = (xs - w / 2) / ax, (ys - h / 2) / ax
    dm = (z * np.sqrt(rx * rx + ry * ry + 1.0)).astype(np.float32)   # ray length
    out = _run(dm, types.SimpleNamespace(flen=flen, R=np.eye(3), t=np.zeros(3)))
    pitch = z / ax
    simple = out["vclass"] == points_ref.VERTEX_CLASS["simple"]
    assert simple.sum() == (w - 2) * (h - 2)
    # four neighbours at one pitch and m = 0..4 across a diagonal (the split
    # of each block follows its depth differences)
    forms = np.array([2.0 * (4.0 + m * np.sqrt(2.0)) / (4.0 + m) * pitch for m in range(5)])
    err = np.abs(out["value"][simple][:, None] / forms[None, :] - 1.0).min(axis=1)
    assert err.max() < 2e-5
    assert np.all(np.isfinite(out["value"]))


def test_ply_round_trip_of_host_writer(tmp_path):
    from smvs_amd import host
    rng = np.random.default_rng(3)
    n = 70000                       # more than one write chunk
    xyz = rng.standard_normal((n, 3)).astype(np.float32)
    nrm = rng.standard_normal((n, 3)).astype(np.float32)
    rgb = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    conf = (rng.integers(0, 5, n) / 4).astype(np.float32)
    val = rng.random(n).astype(np.float32)
    path = str(tmp_path / "points.ply")
    host.save_ply_points(path, xyz, nrm, rgb, conf, val)
    props, names, n_faces, rest = points_ref.read_ply(path)
    assert names == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue",
                     "confidence", "value"]
    assert n_faces == 0 and rest == 0
    assert np.array_equal(np.stack([props["x"], props["y"], props["z"]], 1), xyz)
    assert np.array_equal(np.stack([props["nx"], props["ny"], props["nz"]], 1), nrm)
    assert np.array_equal(np.stack([props["red"], props["green"], props["blue"]], 1), rgb)
    assert np.array_equal(props["confidence"], conf)
    assert np.array_equal(props["value"], val)
    empty = str(tmp_path / "empty.ply")
    host.save_ply_points(empty, xyz[:0], nrm[:0], rgb[:0], conf[:0], val[:0])
    props, _, n_faces, rest = points_ref.read_ply(empty)
    assert len(props["x"]) == 0 and n_faces == 0 and rest == 0
    assert os.path.getsize(empty) > 0
