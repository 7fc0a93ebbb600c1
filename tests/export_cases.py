"""Inputs on which every rule of the export paths decides (DESIGN.md section 9:
P1-P15 of csrc/mesh.hip's point export, M1-M6 of the triangle mesh, S1-S13 of
csrc/simplify.hip) -- plain numpy with fixed seeds, no GPU; walked by
test_export_cases_cpu.py (the floors that make the cases non-vacuous, and the
variants of the restatements that each must catch) and by
test_gpu_export_cases.py (the device against the restatements).

The synthetic sphere in front of a plane with 1 % single-pixel holes hardly
ever reaches a decisive branch.  The cases here:

regular grid (generate_points, generate_mesh), a RUN = case + options
  holes_dense     48 x 40, constant on the left and gently tilted on the
                  right, 35 % zeros: complex, border and simple vertices in
                  hundreds, all 16 corner masks; also with an AABB
  quantised       48 x 40 on the levels 4 + k / 64, k in {0, 1, 2}: a third of
                  the full blocks tie in P2, vertices with 4 and 8 faces
  disc_ladder     161 x 121 of separate 2 x 2 blocks, one triangle each, whose
                  deciding edge steps by the last float below, the float
                  exactly at and the first float above footprint[i_min] *
                  factor (see _disc_ladder), run with dd_factor 0, 0.5, 5, 20
  rings           a 36 x 26 filled region (hop distances 0 to 4 and beyond) with
                  interior complex vertices, which take a ring value (P10)
  mixed_sizes     97 x 63, 2 x 2, 40 x 30, 2 x 57, 1 x 50, 63 x 97, 161 x 121
                  in one call, 1 and 3 channels in turn; with and without the
                  cut, reversed, and with an AABB
  all_holes_view  a view without any depth between two normal ones

simplified (simplify_triangulate, generate_simplified)
  terraces        97 x 63 plateaus in steps of 0.25: equal keys, equal distances
  exhaustive      24 x 16, four levels, max_vertices = w h + 10, max_error = 0:
                  the loop ends in S5 by itself
  limits_*        4096 x 2, 2 x 4096, 2 x 2, 2 x 40, 3 x 300
  hole_blocks     97 x 63 with zero rectangles of 4, 5 and more pixels and
                  zero corner pixels
  slivers         a steep ramp: min_edge / max_edge on both sides of 0.1
  mixed_sizes     the list above without the 1 x 50 view, one view emptied,
                  explicit max_vertices / max_error

A case is (name, cams, depths, normals, images); build it with get(name) and
treat it as read-only.
"""
import collections
import functools

import numpy as np

import cut_ref  # tests/cut_ref.py
import mesh_ref  # tests/mesh_ref.py
import points_ref  # tests/points_ref.py
import simplify_ref  # tests/simplify_ref.py

Case = collections.namedtuple("Case", "name cams depths normals images")
Run = collections.namedtuple("Run", "id case dd_factor cut aabb")
SimplifyRun = collections.namedtuple("SimplifyRun", "id case max_vertices max_error aabb")

TARGET = (0.0, 0.0, 4.0)
FLEN = 1.2
F = np.float32

# (centre, target, width, height, flen)
MIXED_VIEWS = (
    ((0.0, 0.0, 0.0), TARGET, 97, 63, 1.2),
    ((0.1, -0.2, 0.0), TARGET, 2, 2, 0.8),
    ((0.2, -1.2, 0.1), TARGET, 40, 30, 0.7),
    ((-0.3, 0.2, 0.0), TARGET, 2, 57, 1.0),
    ((0.3, 0.2, 0.1), TARGET, 1, 50, 1.2),
    ((1.5, 0.0, 0.3), TARGET, 63, 97, 0.9),
    ((-2.0, 0.4, 1.0), TARGET, 161, 121, 1.6),
)
ONE_COLUMN_VIEW = 4          # the 1 x 50 view: no block, nothing exported
EMPTIED_VIEW = 2             # mixed_sizes_simplified: the 40 x 30 view has no depth

DD_FACTORS = (0.0, 0.5, 5.0, 20.0)


def _camera(centre, target, w, h, flen):
    from smvs_amd import synth
    return synth.Camera(*synth.look_at(centre, target), flen, w, h)


def _ring_camera(w, h):
    """A pose none of whose rotation entries is 0 or 1."""
    return _camera((0.2, 0.1, 0.0), TARGET, w, h, FLEN)


def _dressing(rng, shapes):
    """Camera-space normals (unit, facing the camera) and u8 images, 3 channels
    and 1 in turn: data for P7 / P12, none of it decides anything."""
    normals, images = [], []
    for i, (h, w) in enumerate(shapes):
        n = rng.standard_normal((h, w, 3)).astype(F) * F(0.2) + np.array([0, 0, -1], F)
        normals.append((n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(F))
        images.append(rng.integers(0, 256, (h, w, 3) if i % 2 == 0 else (h, w)).astype(np.uint8))
    return normals, images


def _single(depth, seed):
    d = np.ascontiguousarray(depth, F)
    normals, images = _dressing(np.random.default_rng(seed), [d.shape])
    return [_ring_camera(d.shape[1], d.shape[0])], [d], normals, images


# ------------------------------------------------------------ regular grid
def _holes_dense():
    w, h = 48, 40
    rng = np.random.default_rng(21)
    yy, xx = np.mgrid[0:h, 0:w]
    d = np.where(xx < w // 2, 4.0, 4.0 + 0.002 * (xx - w // 2) + 0.001 * yy).astype(F)
    d[rng.random((h, w)) < 0.35] = 0.0
    return _single(d, 22)


def _quantised():
    w, h = 48, 40
    rng = np.random.default_rng(23)
    d = (4.0 + rng.integers(0, 3, (h, w)) / 64.0).astype(F)
    return _single(d, 24)


def footprints(w, h, flen, xs, ys, d):
    """pixel_footprint (P4) of the restatement in numpy float32, operation by
    operation, for arrays of pixels (test_export_cases_cpu.py holds it against
    points_ref.footprint)."""
    ax = F(flen) * F(max(w, h))
    inv0, inv2, inv5 = F(1) / ax, -F(w) * F(0.5) / ax, -F(h) * F(0.5) / ax
    px, py = xs.astype(F) + F(0.5), ys.astype(F) + F(0.5)
    zero = np.zeros(px.shape, F)
    v0 = ((zero + inv0 * px) + F(0) * py) + inv2 * F(1)
    v1 = ((zero + F(0) * px) + inv0 * py) + inv5 * F(1)
    v2 = ((zero + F(0) * px) + F(0) * py) + F(1) * F(1)
    norm = np.sqrt(((zero + v0 * v0) + v1 * v1) + v2 * v2)
    return (inv0 * d.astype(F)) / norm


def edge_limit(fp, factor, diagonal):
    """P3's right-hand side: footprint[i_min] * factor, the factor times
    MATH_SQRT2 in double and rounded to float on a diagonal."""
    f = F(np.float64(F(factor)) * 1.41421356237309504880) if diagonal else F(factor)
    return fp * f


LADDER_W, LADDER_H, LADDER_PITCH = 161, 121, 3
# the deciding edge of a block: (corner mask, corner pair, the third corner
# takes the depth of: a corner of the pair or "mid")
LADDER_KINDS = (("axis_h", 7, (0, 1), (2, 0)), ("axis_v", 7, (0, 2), (1, 0)),
                ("diag", 11, (0, 3), (1, "mid")), ("anti", 14, (1, 2), (3, "mid")))
LADDER_RUNGS = ("below", "at", "above")
LADDER_BASE = 4.0
LADDER_TRIALS = 1 << 14


@functools.lru_cache(maxsize=None)
def ladder_plan():
    """Per block of the ladder (by, bx): the dd_factor it is built for, its
    kind, its rung and which corner of the pair is the smaller depth; the four
    last entries of every 76 are blocks of four equal depths."""
    nbx, nby = (LADDER_W - 2) // LADDER_PITCH + 1, (LADDER_H - 2) // LADDER_PITCH + 1
    plan = []
    for b in range(nbx * nby):
        c = b % 76
        if c >= 72:
            plan.append((b // nbx, b % nbx, None, None, None, None))
            continue
        factor = DD_FACTORS[1 + c % 3]
        kind = (c // 3) % 4
        rung = (c // 12) % 3
        swap = c // 36
        plan.append((b // nbx, b % nbx, factor, kind, rung, swap))
    return tuple(plan)


def _disc_ladder():
    """Separate 2 x 2 blocks, one triangle each, pitch 3.  A block's deciding
    edge (lo, hi) has depth[lo] = m, about 4, and depth[hi] = m + step; every
    other edge of its triangle is far from its own threshold (the third corner
    repeats a corner of the pair, or lies midway for a diagonal).  The
    subtraction of two floats in [4, 8) is exact and a multiple of 2^-21, so
    `step == footprint[lo] * factor` needs a threshold that is such a multiple:
    m runs over LADDER_TRIALS floats from 4 upward until it is one (the
    footprint is linear in the depth, its low bits are as good as random).
    below = the last float whose step is under the threshold, above = the first
    one over it."""
    w, h = LADDER_W, LADDER_H
    d = np.zeros((h, w), F)
    ulp = F(2.0 ** -21)
    trials = F(LADDER_BASE) + np.arange(LADDER_TRIALS, dtype=F) * ulp
    for by, bx, factor, kind, rung, swap in ladder_plan():
        x, y = LADDER_PITCH * bx, LADDER_PITCH * by
        corner = [(x, y), (x + 1, y), (x, y + 1), (x + 1, y + 1)]
        if factor is None:
            for cx, cy in corner:
                d[cy, cx] = F(LADDER_BASE + 0.25 * ((bx + by) % 3))
            continue
        _, _, pair, (third, source) = LADDER_KINDS[kind]
        lo, hi = pair[::-1] if swap else pair
        lx, ly = corner[lo]
        limit = edge_limit(footprints(w, h, FLEN, np.full(len(trials), lx), np.full(len(trials), ly),
                                      trials), factor, kind >= 2)
        # the largest float step <= limit is a multiple of 2^-21
        exact = np.nonzero(np.floor(limit / ulp) * ulp == limit)[0]
        k = int(exact[0]) if len(exact) else 0
        if LADDER_RUNGS[rung] == "at":
            assert len(exact), "no exact threshold among the trial depths"
        m = trials[k]
        top = F(m + F(np.floor(limit[k] / ulp)) * ulp)          # step <= limit < step + ulp
        assert F(top - m) <= limit[k] < F(F(top + ulp) - m)
        if LADDER_RUNGS[rung] == "below" and F(top - m) == limit[k]:
            top = F(top - ulp)
        elif LADDER_RUNGS[rung] == "above":
            top = F(top + ulp)
        d[corner[lo][1], corner[lo][0]] = m
        d[corner[hi][1], corner[hi][0]] = top
        value = F((np.float64(m) + np.float64(top)) * 0.5) if source == "mid" else \
            d[corner[source][1], corner[source][0]]
        d[corner[third][1], corner[third][0]] = value
    return _single(d, 26)


RINGS_COMPLEX = ((8, 9), (14, 12), (20, 15), (27, 9), (31, 20), (11, 21))      # (x, y)


def _rings():
    w, h = 40, 30
    yy, xx = np.mgrid[0:h, 0:w]
    d = np.zeros((h, w), F)
    d[2:28, 2:38] = (5.0 + 0.003 * xx + 0.002 * yy).astype(F)[2:28, 2:38]
    # a vertex whose left and right neighbours are holes: the two faces above
    # it and the two below it share no edge -- complex, deep inside the region
    for x, y in RINGS_COMPLEX:
        d[y, x - 1] = d[y, x + 1] = 0.0
    return _single(d, 27)


@functools.lru_cache(maxsize=None)
def _scene():
    from smvs_amd import synth
    return synth.pipeline_inputs("sphere", 97, 63, 2, flen=FLEN)["scene"]


def _mixed_sizes():
    from smvs_amd import synth
    cams = [_camera(*v) for v in MIXED_VIEWS]
    depths, normals = synth.depth_and_normal_maps(_scene(), cams)
    rng = np.random.default_rng(31)
    for d in depths:
        d *= (1.0 + 0.002 * rng.standard_normal(d.shape)).astype(F)
        if d.size > 4:
            d[rng.random(d.shape) < 0.03] = 0.0
    _, images = _dressing(rng, [d.shape for d in depths])
    return cams, depths, normals, images


def _all_holes_view():
    from smvs_amd import synth
    main, subs = synth.ring_cameras(64, 48, 2, flen=FLEN)
    cams = [main, subs[0], subs[1]]
    depths, normals = synth.depth_and_normal_maps(_scene(), cams)
    rng = np.random.default_rng(33)
    for d in depths:
        d[rng.random(d.shape) < 0.05] = 0.0
    depths[1][:] = 0.0
    _, images = _dressing(rng, [d.shape for d in depths])
    return cams, depths, normals, images


# --------------------------------------------------------------- simplified
def _terraces():
    w, h = 97, 63
    yy, xx = np.mgrid[0:h, 0:w]
    d = (4.0 + 0.25 * ((xx // 12 + 2 * (yy // 9)) % 4)).astype(F)
    return _single(d, 41)


def _exhaustive():
    w, h = 24, 16
    rng = np.random.default_rng(43)
    d = (4.0 + 0.25 * rng.integers(0, 4, (h, w))).astype(F)
    return _single(d, 44)


LIMIT_SIZES = ((4096, 2), (2, 4096), (2, 2), (2, 40), (3, 300))     # (w, h)


def _limits(w, h):
    rng = np.random.default_rng(45 + w + h)
    d = (4.0 + 0.25 * rng.integers(0, 3, (h, w))).astype(F)
    return _single(d, 46)


def _hole_blocks():
    w, h = 97, 63
    rng = np.random.default_rng(47)
    yy, xx = np.mgrid[0:h, 0:w]
    d = (4.0 + 0.3 * np.sin(xx / 9.0) * np.cos(yy / 7.0)).astype(F)
    d *= (1.0 + 0.002 * rng.standard_normal((h, w))).astype(F)
    # 2 x 2 (4 pixels) and 1 x 5 (5 pixels) on a jittered lattice, then a few
    # larger rectangles
    for by in range(3, h - 6, 8):
        for bx in range(3, w - 8, 9):
            x, y = bx + int(rng.integers(0, 3)), by + int(rng.integers(0, 3))
            if (bx // 9 + by // 8) % 2:
                d[y:y + 2, x:x + 2] = 0.0
            else:
                d[y, x:x + 5] = 0.0
    for x, y, bw, bh in ((20, 10, 7, 3), (60, 30, 3, 9), (40, 45, 11, 6), (80, 8, 5, 5)):
        d[y:y + bh, x:x + bw] = 0.0
    d[0, 0] = d[0, w - 1] = d[h - 1, 0] = d[h - 1, w - 1] = 0.0        # S3: dm_max
    return _single(d, 48)


def _slivers():
    w, h = 64, 48
    rng = np.random.default_rng(49)
    yy, xx = np.mgrid[0:h, 0:w]
    # the depth grows by 8 % per column, 6 pixel footprints: an edge along x is
    # that much longer in the world than one along y, at every depth
    d = (2.0 * np.exp(0.08 * xx) * (1.0 + 0.004 * rng.standard_normal((h, w)))).astype(F)
    return _single(d, 50)


def _mixed_sizes_simplified():
    cams, depths, normals, images = [list(p) for p in get("mixed_sizes")[1:]]
    for part in (cams, depths, normals, images):
        del part[ONE_COLUMN_VIEW]
    depths[EMPTIED_VIEW] = np.zeros_like(depths[EMPTIED_VIEW])
    return cams, depths, normals, images


_BUILDERS = {"holes_dense": _holes_dense, "quantised": _quantised, "disc_ladder": _disc_ladder,
             "rings": _rings, "mixed_sizes": _mixed_sizes, "all_holes_view": _all_holes_view,
             "terraces": _terraces, "exhaustive": _exhaustive, "hole_blocks": _hole_blocks,
             "slivers": _slivers, "mixed_sizes_simplified": _mixed_sizes_simplified}
for _w, _h in LIMIT_SIZES:
    _BUILDERS["limits_%dx%d" % (_w, _h)] = functools.partial(_limits, _w, _h)

REGULAR_NAMES = ("holes_dense", "quantised", "disc_ladder", "rings", "mixed_sizes",
                 "mixed_sizes_reversed", "all_holes_view")
SIMPLIFY_NAMES = ("terraces", "exhaustive") + tuple("limits_%dx%d" % s for s in LIMIT_SIZES) + (
    "hole_blocks", "slivers", "mixed_sizes_simplified")


@functools.lru_cache(maxsize=None)
def get(name):
    if name == "mixed_sizes_reversed":
        return Case(name, *[list(reversed(part)) for part in get("mixed_sizes")[1:]])
    cams, depths, normals, images = _BUILDERS[name]()
    depths = [np.ascontiguousarray(d, F) for d in depths]
    normals = [np.ascontiguousarray(n, F) for n in normals]
    return Case(name, list(cams), depths, normals, list(images))


def maps(name, oracle=None):
    """The maps the export triangulates and the world normals it looks up:
    without an oracle the input maps (cut=False; the normals by cut_ref, which
    test_cut_cases_cpu.py holds equal to the oracle's), with one the oracle's
    cut of the whole list."""
    c = get(name)
    if oracle is not None:
        return oracle.cut_depth_maps(c.cams, c.depths, c.normals)
    wn = [cut_ref.View(cam, d.shape[1], d.shape[0]).world_normals(n)
          for cam, d, n in zip(c.cams, c.depths, c.normals)]
    return c.depths, wn


@functools.lru_cache(maxsize=None)
def aabb(name):
    """A box that cuts through the faces of every view that has any: for the
    mixed list one through the sphere's front, the noisy plane at z = 8 and the
    two-column view; else the 25th to the 80th percentile of the unclipped
    vertices."""
    if name == "mixed_sizes":
        return (-0.8, -0.45, 2.0), (0.15, 0.6, 8.0)
    dms, wn = maps(name)
    c = get(name)
    full = points_ref.points(c.cams, dms, wn, c.images)
    lo = np.percentile(full["xyz"], 25, axis=0).astype(F)
    hi = np.percentile(full["xyz"], 80, axis=0).astype(F)
    return tuple(float(v) for v in lo), tuple(float(v) for v in hi)


def _regular_runs():
    runs = [Run("holes_dense", "holes_dense", 5.0, False, False),
            Run("holes_dense-aabb", "holes_dense", 5.0, False, True),
            Run("quantised", "quantised", 5.0, False, False)]
    runs += [Run("disc_ladder-dd%g" % f, "disc_ladder", f, False, False) for f in DD_FACTORS]
    runs += [Run("rings", "rings", 5.0, False, False),
             Run("mixed_sizes", "mixed_sizes", 5.0, False, False),
             Run("mixed_sizes-aabb", "mixed_sizes", 5.0, False, True),
             Run("mixed_sizes-cut", "mixed_sizes", 5.0, True, False),
             Run("mixed_sizes_reversed-cut", "mixed_sizes_reversed", 5.0, True, False),
             Run("all_holes_view", "all_holes_view", 5.0, False, False)]
    return tuple(runs)


def _simplify_runs():
    runs = [SimplifyRun("terraces", "terraces", -1, -1.0, False),
            SimplifyRun("exhaustive", "exhaustive", 24 * 16 + 10, 0.0, False)]
    runs += [SimplifyRun("limits_%dx%d" % s, "limits_%dx%d" % s, -1, -1.0, False)
             for s in LIMIT_SIZES]
    runs += [SimplifyRun("hole_blocks", "hole_blocks", -1, -1.0, False),
             SimplifyRun("slivers", "slivers", -1, -1.0, False),
             SimplifyRun("mixed_sizes_simplified", "mixed_sizes_simplified", 60, 0.002, False),
             SimplifyRun("mixed_sizes_simplified-aabb", "mixed_sizes_simplified", 60, 0.002, True)]
    return tuple(runs)


REGULAR_RUNS = _regular_runs()
SIMPLIFY_RUNS = _simplify_runs()
# the runs whose maps are not cut: a restatement alone gives their reference
UNCUT_RUNS = tuple(r for r in REGULAR_RUNS if not r.cut)


def box(run):
    if not run.aabb:
        return None
    return aabb("mixed_sizes" if run.case.startswith("mixed_sizes") else run.case)


def normals_f64(xyz, faces):
    """M3-M5 (recalc_normals) in float64 numpy from float positions and faces:
    what both float implementations approximate.  A vertex on nearly opposite
    faces has a short sum, and the rounding of the float weights then shows in
    its normal well above 1e-6 on either side."""
    x = np.asarray(xyz, np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    vn = np.zeros_like(x)
    if len(f):
        a, b, c = x[f[:, 0]], x[f[:, 1]], x[f[:, 2]]
        ab, bc, ca = b - a, c - b, a - c
        fn = np.cross(ab, -ca)
        fnl = np.linalg.norm(fn, axis=1)
        ok = fnl > 0

        def angle(u, v):
            with np.errstate(all="ignore"):
                cos = (u * v).sum(axis=1) / (np.linalg.norm(u, axis=1) * np.linalg.norm(v, axis=1))
            return np.arccos(np.clip(cos, -1.0, 1.0))
        weights = (angle(ab, -ca), angle(-ab, bc), angle(ca, -bc))
        with np.errstate(all="ignore"):
            fn = fn / fnl[:, None]
        for corner, w in enumerate(weights):
            np.add.at(vn, f[ok, corner], fn[ok] * w[ok, None])
    length = np.linalg.norm(vn, axis=1)
    with np.errstate(all="ignore"):
        return np.where(length[:, None] > 0, vn / length[:, None], 0.0)


def normal_deviation(mesh):
    """max |normal - float64 normal| over the vertices of a mesh dict that have
    a normal there (the zero normals are compared exactly elsewhere)."""
    n = mesh["normals"].astype(np.float64)
    has = np.any(n != 0, axis=1)
    if not has.any():
        return 0.0
    return float(np.abs(n - normals_f64(mesh["xyz"], mesh["faces"]))[has].max())


_CACHE = {}


def restated_points(run, variant=None, oracle=None):
    """points_ref.points of a regular run (read-only; variant None is cached)."""
    key = ("points", run.id, variant)
    if key not in _CACHE:
        c = get(run.case)
        dms, wn = maps(run.case, oracle if run.cut else None)
        _CACHE[key] = points_ref.points(c.cams, dms, wn, c.images, aabb=box(run),
                                        dd_factor=run.dd_factor, variant=variant)
    return _CACHE[key]


def restated_mesh(run, variant=None, oracle=None):
    key = ("mesh", run.id, variant)
    if key not in _CACHE:
        c = get(run.case)
        dms, wn = maps(run.case, oracle if run.cut else None)
        _CACHE[key] = mesh_ref.mesh(c.cams, dms, wn, c.images, aabb=box(run),
                                    dd_factor=run.dd_factor, variant=variant)
    return _CACHE[key]


def restated_triangulation(run, view=0, variant=None):
    key = ("tri", run.id, view, variant)
    if key not in _CACHE:
        _CACHE[key] = simplify_ref.triangulate(get(run.case).depths[view], run.max_vertices,
                                               run.max_error, variant=variant)
    return _CACHE[key]


def restated_simplified(run, mesh, variant=None):
    key = ("simplified", run.id, bool(mesh), variant)
    if key not in _CACHE:
        c = get(run.case)
        dms, wn = maps(run.case)
        _CACHE[key] = simplify_ref.simplified(c.cams, dms, wn, c.images, mesh=mesh,
                                              aabb=box(run), max_vertices=run.max_vertices,
                                              max_error=run.max_error, variant=variant)
    return _CACHE[key]
