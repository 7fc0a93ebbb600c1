"""Known answers of smvsrecon --simplify's semantics (DESIGN.md section 9.7,
S1-S13) that do not depend on the restatement being right: the Delaunay
triangulation checked in Python integers, the rasteriser against an
enumeration written from row S8, the heap order, properties of the greedy
loop, the clean-up's quirks, and the new entries.  No GPU."""
import math
import types

import numpy as np
import pytest

import simplify_ref  # tests/simplify_ref.py

IDENT = types.SimpleNamespace(flen=1.0, R=np.eye(3, dtype=np.float32),
                              t=np.zeros(3, np.float32))


def _area2(a, b, c):
    return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])


def _in_circle(a, b, c, p):
    sq = lambda q: q[0] * q[0] + q[1] * q[1]
    return (sq(a) * _area2(b, c, p) - sq(b) * _area2(a, c, p) + sq(c) * _area2(a, b, p)
            - sq(p) * _area2(a, b, c))


def test_spiral_gives_the_euler_count_of_triangles():
    # 15 points in [-4, 4]^2 plus the 4 corners: 2 * 19 - 2 - 4 = 32 triangles
    pts = [(0.25 * i + 0.2) * np.array([math.cos(0.9 * i), math.sin(0.9 * i)])
           for i in range(15)]
    nv, tris, changed = simplify_ref.delaunay(pts, -4, 4)
    assert nv == 19 and len(tris) == 32
    assert changed.min() >= 4   # the two new triangles, the old one, and flips


@pytest.mark.parametrize("seed,n,size", [(0, 40, 16), (1, 200, 64), (2, 300, 20)])
def test_random_integer_points_are_delaunay(seed, n, size):
    rng = np.random.default_rng(seed)
    pts = [tuple(int(v) for v in p) for p in rng.integers(0, size, (n, 2))]
    nv, tris, changed = simplify_ref.delaunay(pts, -1, size)
    verts = [(-1, -1), (size, -1), (-1, size), (size, size)]
    for p, c in zip(pts, changed):
        # S5: a repeated point changes nothing
        assert (c == 0) == (p in verts)
        if c:
            verts.append(p)
    assert nv == len(verts) and len(tris) == 2 * nv - 2 - 4
    for t in tris:
        # S4 lists a triangle's vertices with l_prev, i.e. against the face's
        # counter-clockwise cycle: reversed, the triple is that cycle
        a, c, b = (verts[i] for i in t)
        assert _area2(a, b, c) > 0                      # counter-clockwise
        for p in verts:
            assert _in_circle(a, b, c, p) <= 0          # nobody strictly inside
    # every triangle once, every vertex used
    assert len({tuple(sorted(t)) for t in tris.tolist()}) == len(tris)
    assert set(tris.ravel().tolist()) == set(range(nv))


def test_point_on_an_edge_and_repeated_point():
    # (2, 2) lies on the quad's diagonal (4, 0)-(0, 4): both triangles are
    # split, the diagonal is replaced (S4 on_edge); again -> S5
    nv, tris, changed = simplify_ref.delaunay([(2, 2), (2, 2), (1, 1)], 0, 4)
    assert changed.tolist()[:2] == [4, 0]
    assert nv == 6 and len(tris) == 6
    assert changed[2] >= 3


def _pixels_from_the_table(a, b, c):
    """Row S8 written out in Python."""
    v = sorted([a, b, c], key=lambda p: p[1])   # stable
    out = []

    def top_flat(a, b, c):
        d1, d2 = (a[0] - c[0]) / (a[1] - c[1]), (a[0] - b[0]) / (a[1] - b[1])
        x1 = x2 = float(a[0])
        y = int(a[1])
        while y <= b[1]:
            out.extend((x, y) for x in range(math.ceil(min(x1, x2)),
                                             math.floor(max(x1, x2)) + 1))
            x1 += d1
            x2 += d2
            y += 1

    def bottom_flat(a, b, c):
        d1, d2 = (c[0] - a[0]) / (c[1] - a[1]), (c[0] - b[0]) / (c[1] - b[1])
        x1 = x2 = float(c[0])
        y = int(c[1])
        while y > b[1]:
            out.extend((x, y) for x in range(math.ceil(min(x1, x2)),
                                             math.floor(max(x1, x2)) + 1))
            x1 -= d1
            x2 -= d2
            y -= 1

    if v[1][1] == v[2][1]:
        top_flat(*v)
    elif v[0][1] == v[1][1]:
        bottom_flat(*v)
    else:
        mx = v[0][0] + ((v[1][1] - v[0][1]) / (v[2][1] - v[0][1])) * (v[2][0] - v[0][0])
        m = (math.ceil(mx) if v[0][0] < v[1][0] else math.floor(mx), v[1][1])
        top_flat(v[0], v[1], m)
        bottom_flat(v[1], m, v[2])
    return out


@pytest.mark.parametrize("tri", [
    ((0, 0), (4, 0), (0, 4)),            # bottom-flat
    ((0, 4), (2, 0), (4, 4)),            # top-flat
    ((0, 0), (6, 3), (1, 7)),            # split, middle vertex right
    ((5, 0), (0, 2), (4, 9)),            # split, middle vertex left
    ((-1, -1), (9, -1), (-1, 9)),        # the first triangle of a 9 x 9 map
    ((3, 1), (7, 5), (2, 6)), ((0, 0), (0, 10), (1, 10))])
def test_rasteriser_against_the_table(tri):
    got = [tuple(p) for p in simplify_ref.pixels(*tri).tolist()]
    assert got == _pixels_from_the_table(*tri)
    assert len(got) == len(set(got)) > 0


def test_rasteriser_adds_dx_repeatedly():
    # dx = 0.1: ten additions give 0.9999999999999999, 10 * 0.1 gives 1.0, so
    # the pixel (1, 10) is left out although the vertex (1, 10) is on its row
    got = [tuple(p) for p in simplify_ref.pixels((0, 0), (0, 10), (1, 10)).tolist()]
    assert (1, 10) not in got and (0, 10) in got
    assert sum(0.1 for _ in range(10)) < 1.0 == 10 * 0.1
    # the bottom row of a bottom-flat triangle is never visited (y > b.y)
    assert all(y > 0 for _, y in simplify_ref.pixels((0, 0), (4, 0), (0, 4)).tolist())


def test_heap_hands_out_equal_keys_in_scan_order():
    assert simplify_ref.heap_order([1, 3, 3, 2, 3]).tolist() == [1, 2, 4, 3, 0]
    assert simplify_ref.heap_order([0, 0, 0]).tolist() == [0, 1, 2]
    big = np.finfo(np.float64).max
    assert simplify_ref.heap_order([5.0, big, 5.0, big]).tolist() == [1, 3, 0, 2]


def _max_error(dm):
    """S2 in numpy's float32, the sum in memory order."""
    flat = dm.ravel()
    avg, counter = np.float32(0), np.float32(0)
    for v in flat[flat > 0]:
        avg = np.float32(avg + v)
        counter = np.float32(counter + np.float32(1))
    avg = np.float32(avg / counter)
    return float(np.float32(flat.max() - avg)) * 1e-3


def test_cone_inserts_the_apex_first():
    yy, xx = np.mgrid[0:9, 0:9]
    dm = (10.0 - np.hypot(xx - 4.0, yy - 4.0)).astype(np.float32)
    r = simplify_ref.triangulate(dm, max_vertices=1)
    assert r["iterations"] == 1
    # the corners take the depth of the nearest pixel (S3)
    assert np.array_equal(r["vertices"][:4], [[-1, -1, dm[0, 0]], [9, -1, dm[0, 8]],
                                              [-1, 9, dm[8, 0]], [9, 9, dm[8, 8]]])
    assert np.array_equal(r["vertices"][4], [4, 4, 10])
    # (4, 4) is on the diagonal: on_edge, four triangles
    assert len(r["triangles"]) == 4


def test_loop_ends_within_the_error_bound():
    yy, xx = np.mgrid[0:25, 0:33]
    dm = (4.0 + 0.02 * np.abs(xx - 14.0) + 0.01 * np.abs(yy - 11.0)).astype(np.float32)
    dm[3:6, 20:24] = 0.0
    r = simplify_ref.triangulate(dm)
    budget = 33 * 25 // 40
    assert 0 < r["iterations"] < budget                   # not exhausted
    assert len(r["vertices"]) == 4 + r["iterations"]      # no no-op insertion here
    bound = _max_error(dm)
    checked = 0
    for t, nz in zip(r["triangles"], r["num_zero_depths"]):
        p = r["vertices"][t]
        n = np.cross(p[1] - p[0], p[2] - p[0])
        n /= np.linalg.norm(n)
        zeros = 0
        for x, y in _pixels_from_the_table(*[tuple(q[:2]) for q in p]):
            if not (0 <= x < 33 and 0 <= y < 25):
                continue
            if dm[y, x] == 0:
                zeros += 1
                continue
            assert abs(np.dot(n, np.array([x, y, dm[y, x]]) - p[0])) < bound + 1e-12
            checked += 1
        assert zeros == nz
    assert checked > 33 * 25 // 2


def test_all_zero_map_contributes_nothing():
    zero = np.zeros((20, 30), np.float32)
    r = simplify_ref.triangulate(zero)
    # (0, 0, 0) once, then no-op insertions through the budget (S1, S5)
    assert r["iterations"] == 15 and len(r["vertices"]) == 5
    assert np.array_equal(r["vertices"][4], [0, 0, 0])
    v = simplify_ref.view(IDENT, zero, np.zeros((20, 30, 3), np.float32),
                          np.zeros((20, 30), np.uint8))
    assert len(v["xyz"]) == 0 and len(v["faces"]) == 0


def test_constant_small_map_contributes_nothing():
    # 64 x depth 2: dm_avg is exactly 2, max_error 0, budget 64 / 40 = 1; the
    # one iteration inserts the candidate of a scan without a distance, (0, 0,
    # 0), and every face touches a corner
    const = np.full((8, 8), 2.0, np.float32)
    assert _max_error(const) == 0.0
    r = simplify_ref.triangulate(const)
    assert r["iterations"] == 1 and np.array_equal(r["vertices"][4], [0, 0, 0])
    assert all((t < 4).any() for t in r["triangles"])
    v = simplify_ref.view(IDENT, const, np.zeros((8, 8, 3), np.float32),
                          np.zeros((8, 8), np.uint8))
    assert len(v["xyz"]) == 0 and len(v["faces"]) == 0


def test_bad_face_test_reads_the_k_th_triangle():
    """S10: face k of the list after the corner deletion is tested against the
    zero count of TRIANGLE k.  On a map with a block of zeros the two readings
    give different face counts, and the restatement's is the reference's."""
    yy, xx = np.mgrid[0:40, 0:56]
    dm = (5.0 + 0.6 * np.sin(xx * 0.21) * np.cos(yy * 0.17)).astype(np.float32)
    dm[14:26, 20:38] = 0.0
    r = simplify_ref.triangulate(dm)
    tris, nz = r["triangles"], r["num_zero_depths"]
    kept = np.nonzero((tris >= 4).all(axis=1))[0]
    assert 0 < len(kept) < len(tris) and not np.array_equal(kept, np.arange(len(kept)))
    # positions as S9 makes them (identity camera), in float32
    v = r["vertices"][4:].astype(np.float32)
    a = np.float32(1.0) / (np.float32(1.0) * np.float32(56))
    ray = np.stack([a * (v[:, 0] + np.float32(0.5)) + np.float32(-28.0) * a,
                    a * (v[:, 1] + np.float32(0.5)) + np.float32(-20.0) * a,
                    np.ones(len(v), np.float32)], 1).astype(np.float32)
    pos = ray / np.linalg.norm(ray, axis=1, keepdims=True).astype(np.float32) * v[:, 2:3]
    f = tris[kept] - 4
    e = [np.linalg.norm(pos[f[:, i]] - pos[f[:, j]], axis=1) for i, j in ((0, 1), (0, 2), (1, 2))]
    ratio = np.minimum.reduce(e) / np.maximum.reduce(e)
    assert np.abs(ratio - 0.1).min() > 1e-3      # no face near the edge-ratio bound
    as_reference = (nz[:len(kept)] > 4) | (ratio < 0.1)
    own_triangle = (nz[kept] > 4) | (ratio < 0.1)
    assert (as_reference != own_triangle).any()
    out = simplify_ref.view(IDENT, dm, np.zeros((40, 56, 3), np.float32),
                            np.zeros((40, 56), np.uint8))
    assert len(out["faces"]) == int((~as_reference).sum()) != int((~own_triangle).sum())


def test_delete_invalid_faces_moves_faces_from_the_end():
    f = [[1, 2, 3], [0, 0, 0], [4, 5, 6], [0, 0, 0], [7, 8, 9], [1, 1, 1], [3, 4, 5]]
    # slot 1 <- the last valid face, slot 3 <- the one before: order NOT kept
    assert simplify_ref.delete_invalid_faces(f).tolist() == \
        [[1, 2, 3], [3, 4, 5], [4, 5, 6], [7, 8, 9]]
    assert simplify_ref.delete_invalid_faces([[0, 0, 0], [2, 2, 2]]).tolist() == []
    assert simplify_ref.delete_invalid_faces([[1, 2, 3], [2, 3, 4]]).tolist() == \
        [[1, 2, 3], [2, 3, 4]]
    assert simplify_ref.delete_invalid_faces([[5, 5, 5], [1, 2, 3]]).tolist() == [[1, 2, 3]]
    # the parallel form of the kernel: the j-th invalid slot among the first
    # n_valid receives the j-th valid face from the end
    rng = np.random.default_rng(4)
    for _ in range(50):
        m = int(rng.integers(1, 40))
        faces = np.stack([np.arange(m) * 3 + 1, np.arange(m) * 3 + 2, np.arange(m) * 3 + 3], 1)
        bad = rng.random(m) < 0.4
        faces[bad] = 0
        n_valid = int((~bad).sum())
        want = faces[:n_valid].copy()
        slots = np.nonzero(bad[:n_valid])[0]
        tail = np.nonzero(~bad[n_valid:])[0][::-1] + n_valid
        want[slots] = faces[tail]
        assert np.array_equal(simplify_ref.delete_invalid_faces(faces), want)


def test_simplify_entries_are_declared_and_exported():
    from smvs_amd import _capi, host
    import smvs_amd
    for name in ("smvs_simplified_generate", "smvs_simplify_triangulate"):
        assert name in _capi.declared_symbols()
        assert hasattr(_capi.load(), name)
    assert "generate_simplified" in smvs_amd.__all__
    assert "simplify_triangulate" in smvs_amd.__all__
    assert hasattr(host.load(), "smvs_host_generate_simplified")
    assert callable(host.generate_simplified)


def test_simplify_entries_refuse_bad_arguments_before_any_work(tmp_path):
    import smvs_amd
    from smvs_amd import host
    from smvs_amd._capi import SmvsError
    ok = np.ones((8, 8), np.float32)
    for bad in (np.ones((1, 40), np.float32), np.ones((40, 1), np.float32),
                np.ones((2, 4097), np.float32)):
        with pytest.raises(SmvsError, match="depth map"):
            smvs_amd.simplify_triangulate(bad)
    for value in (np.nan, np.inf, -1.0):
        d = ok.copy()
        d[3, 3] = value
        with pytest.raises(SmvsError, match="finite"):
            smvs_amd.simplify_triangulate(d)
        with pytest.raises(SmvsError, match="finite"):
            smvs_amd.generate_simplified([IDENT], [d], [np.zeros((8, 8, 3), np.float32)],
                                         [np.zeros((8, 8), np.uint8)])
    with pytest.raises(SmvsError, match="max_vertices"):
        smvs_amd.simplify_triangulate(ok, max_vertices=-2)
    with pytest.raises(SmvsError, match="max_error"):
        smvs_amd.simplify_triangulate(ok, max_error=-0.5)
    with pytest.raises(ValueError):   # image size != depth size (P7)
        smvs_amd.generate_simplified([IDENT], [ok], [np.zeros((8, 8, 3), np.float32)],
                                     [np.zeros((8, 7), np.uint8)])
    with pytest.raises(SmvsError):    # no scene there
        host.generate_simplified(str(tmp_path / "nothing"))
