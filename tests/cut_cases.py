"""View sets on which every branch of the cross-view cut (csrc/mesh_cut.hip:
mesh_prepare_kernel, mesh_cut_kernel) decides -- plain numpy, no GPU; walked
by test_cut_cases_cpu.py (the restatement tests/cut_ref.py against the oracle,
and the tallies that make the cases non-vacuous) and by test_gpu_cut_cases.py
(the device against the oracle, and the exports that read the cut maps).

synth.pipeline_inputs gives cameras on a small ring that all look at one
target with one size and focal length: nothing is ever behind a camera, hardly
anything meets a hole, and no view differs in size.  The cases here:

  mixed_wide        six views of the sphere scene with sizes from 33 x 47 to
                    161 x 121 (portrait and landscape), focal lengths 0.7 to
                    1.6, a wide baseline and one camera that faces away; 0.2 %
                    noise, 2 % holes: all eight outcomes of a (pixel, view) pair
  mixed_wide_reversed  the same list backwards: the `break` changes which later
                    views a pixel ever looks at
  threshold_ladder  two views of one pose; depth_1 = depth_0 * r, r = 1 / 1.01
                    on the left half and 1 / 0.997 on the right, moved by
                    -4 .. 4 float ulps: pixels on both sides of the two depth
                    thresholds, some of which a float comparison would flip
  power_ladder      the same pair and a third view of that pose which adds a
                    quarter of the pixel's power; normals_1 = normals_0 * s with s = 2 -4 .. 4
                    ulps on the left half (the `break`) and, on the right half,
                    depth_1 = depth_0 / 0.99 (view 1 in front) with s about
                    0.51 -4 .. 4 ulps, where power_j_j meets 0.5 * power (the
                    subtraction).  2 * power and 0.5 * power are exact
                    in float unless they overflow or are subnormal, so two
                    bands of rows hold normals at those ends of the float range
                    (see _power_ladder): there alone can a float comparison of
                    the power thresholds differ from the reference's double one
  backfacing        three ring views; a block of view 0 has its normals
                    negated (power < 0: cut, yet walked, and still pos_j)
  behind_camera     two ring views and, between them, a camera beyond the scene
                    that faces away: every point is behind it, and its mirror
                    image lands on a pixel that would be subtracted
  principal_plane   view 0 at the identity pose; view 1's centre is the float
                    world point of a pixel of view 0 (proj = (0, 0, 0) there),
                    view 2's centre lies in the principal plane through a
                    second pixel (proj[2] = 0, proj[0] != 0); a ring view keeps
                    both pixels, so a pair that is not skipped shows
  degenerate_sizes  a 2 x 2 view, an all-zero map and a 1 x 300 view between two
                    97 x 63 views

A case is (name, cams, depths, normals, images); build it with get(name) and
treat it as read-only.
"""
import collections
import functools

import numpy as np

import cut_ref  # tests/cut_ref.py

Case = collections.namedtuple("Case", "name cams depths normals images")

NAMES = ("mixed_wide", "mixed_wide_reversed", "threshold_ladder", "power_ladder", "backfacing",
         "behind_camera", "principal_plane", "degenerate_sizes")
LADDER = np.arange(-4, 5)
W, H, FLEN = 97, 63, 1.2
TARGET = (0.0, 0.0, 4.0)

# (centre, target, width, height, flen)
MIXED_VIEWS = (
    ((0.0, 0.0, 0.0), TARGET, 97, 63, 1.2),
    ((1.5, 0.0, 0.3), TARGET, 63, 97, 0.9),
    ((-2.0, 0.4, 1.0), TARGET, 161, 121, 1.6),
    ((0.2, -1.2, 0.1), TARGET, 40, 30, 0.7),
    ((0.1, 0.1, -0.5), (0.1, 0.1, -5.0), 33, 47, 1.2),      # faces away
    ((0.3, 0.0, 0.0), TARGET, 97, 63, 1.2),
)
# principal_plane: the two pixels (x, y) of view 0 and the shift of view 2's
# centre inside its principal plane
PLANE_PIXELS = ((32, 24), (20, 30))
PLANE_SHIFT = 0.125


@functools.lru_cache(maxsize=None)
def _scene():
    from smvs_amd import synth
    return synth.pipeline_inputs("sphere", W, H, 2, flen=FLEN)["scene"]


def _camera(centre, target, w, h, flen):
    from smvs_amd import synth
    return synth.Camera(*synth.look_at(centre, target), flen, w, h)


def _images(rng, depths):
    """u8 noise, 3 channels and 1 in turn."""
    return [rng.integers(0, 256, d.shape + (3,) if i % 2 == 0 else d.shape).astype(np.uint8)
            for i, d in enumerate(depths)]


def _ulps(a, k):
    """a moved by k float32 ulps (k an integer array of a's shape)."""
    a = np.array(a, np.float32)
    for step in range(1, int(np.abs(k).max()) + 1):
        up, down = k >= step, k <= -step
        a[up] = np.nextafter(a[up], np.float32(np.inf))
        a[down] = np.nextafter(a[down], np.float32(-np.inf))
    return a


def _rungs(h, w):
    """k = -4 .. 4 running over the pixels."""
    return LADDER[np.arange(h * w).reshape(h, w) % len(LADDER)]


def _mixed_wide():
    from smvs_amd import synth
    cams = [_camera(*v) for v in MIXED_VIEWS]
    depths, normals = synth.depth_and_normal_maps(_scene(), cams)
    rng = np.random.default_rng(3)
    for d in depths:
        d *= (1.0 + 0.002 * rng.standard_normal(d.shape)).astype(np.float32)
        d[rng.random(d.shape) < 0.02] = 0.0
    return cams, depths, normals, _images(rng, depths)


def _ladder_pair():
    """Two cameras of one pose and size (a ring position, so that no entry of
    the rotation is 0 or 1) with the scene's maps for both."""
    from smvs_amd import synth
    cam = _camera((0.2, 0.1, 0.0), TARGET, W, H, FLEN)
    twin = synth.Camera(cam.R.copy(), cam.t.copy(), FLEN, W, H)
    depths, normals = synth.depth_and_normal_maps(_scene(), [cam])
    return [cam, twin], depths[0], normals[0]


def _threshold_ladder():
    cams, d0, n0 = _ladder_pair()
    r = np.where(np.arange(W) < W // 2, np.float32(1.0) / np.float32(1.01),
                 np.float32(1.0) / np.float32(0.997)).astype(np.float32)
    d1 = _ulps(d0 * r[None, :], _rungs(H, W))
    rng = np.random.default_rng(11)
    return cams, [d0, d1], [n0, n0.copy()], _images(rng, [d0, d1])


# power_ladder: the rows whose normals sit at the ends of the float range
SUBNORMAL_ROWS = slice(4, 16)
OVERFLOW_ROWS = slice(40, 52)


def _power_ladder():
    """normals_1 = normals_0 * s (the reference never normalises a normal and
    the surface power is linear in it, so power_j_j / power = s up to rounding).

    Left half: s = 2 -4 .. 4 ulps at equal depths.  Right half: depth_1 =
    depth_0 / 0.99, so that view 0 finds view 1 in front, and s -4 .. 4 ulps
    around the factor at which power_j_j = 0.5 * power (about 0.51); the third
    view makes that decision show in view 0's map.

    Multiplying a float by 2.0 or 0.5 is exact unless the result overflows or
    is subnormal; only there can `power_j_j > 2.0f * power` differ from the
    double comparison.  Two bands make those operands: both views are given the
    depth at which a pixel is about one world unit wide (the cross product of
    get_surface_power is then about 1.2 resp. 1) and fronto-parallel normals
      OVERFLOW_ROWS, left half   n_1 = 0.95 FLT_MAX, n_0 = n_1 / s: power_j_j
                                 overflows to +inf, power is finite, 2 * power
                                 is finite in double and +inf in float
      SUBNORMAL_ROWS, right half n_0 = m and n_1 = (m + 1) / 2 + k units of
                                 2^-149 with m = 3 mod 4: 0.5 * power is a tie
                                 that float rounds up to (m + 1) / 2
    """
    cams, d0, n0 = _ladder_pair()
    d0, n0 = d0.copy(), n0.copy()
    left = np.broadcast_to(np.arange(W) < W // 2, (H, W))
    k = _rungs(H, W)
    d1 = np.where(left, d0, d0 / np.float32(0.99)).astype(np.float32)
    # view 1's point lies 1 % behind the pixel's own, where the power of the
    # same normal is about 2 % smaller: s = 0.5 * power(pos) / power(pos_j),
    # about 0.51, is the factor at which power_j_j meets 0.5 * power
    view = cut_ref.View(cams[0], W, H)
    ys, xs = np.mgrid[0:H, 0:W]
    wn0 = view.world_normals(n0)
    half = (0.5 * view.surface_power(view.world_point(xs, ys, d0), wn0).astype(np.float64)
            / view.surface_power(view.world_point(xs, ys, d1), wn0)).astype(np.float32)
    s = np.where(left, _ulps(np.full((H, W), 2.0, np.float32), k), _ulps(half, k))
    n1 = n0 * s[..., None]

    _, length = view.rays(xs, ys)
    ax = view.K[0, 0]
    tiny = np.float32(2.0 ** -149)
    big = np.float32(0.95) * np.finfo(np.float32).max

    rows = np.zeros((H, W), bool)
    rows[OVERFLOW_ROWS] = True
    band = rows & left
    # z = ax / sqrt(1.2): (ax / z)^2 = 1.2
    d0[band] = (ax / np.float32(np.sqrt(1.2)) * length)[band]
    d1[band] = d0[band]
    n1[band] = np.stack([0 * s, 0 * s, 0 * s + big], -1)[band]
    n0[band] = (n1[..., 2] / s)[band][:, None] * np.array([0, 0, 1], np.float32)

    rows = np.zeros((H, W), bool)
    rows[SUBNORMAL_ROWS] = True
    band = rows & ~left
    # view 1's point, 1 / 0.99 further away, is the one at (ax / z)^2 = 1
    d1[band] = (ax * length)[band]
    d0[band] = (d1 * np.float32(0.99))[band]
    m = (3 + 4 * ((xs + 3 * ys) % 6)).astype(np.float32)            # 3, 7 .. 23
    n0[band] = ((m * tiny)[..., None] * np.array([0, 0, 1], np.float32))[band]
    n1[band] = ((((m + 1) / 2 + k) * tiny)[..., None] * np.array([0, 0, 1], np.float32))[band]
    # With two views a subtraction changes no map: the sum is negative with it
    # and zero without, cut either way.  A third view of the same pose, at view
    # 0's depths with a quarter of its normals, adds a quarter of the power:
    # view 0's pixel is kept unless view 1 is subtracted.
    from smvs_amd import synth
    cams = cams + [synth.Camera(cams[0].R.copy(), cams[0].t.copy(), FLEN, W, H)]
    n2 = n0 * np.float32(0.25)
    rng = np.random.default_rng(12)
    depths = [d0, d1, d0.copy()]
    return cams, depths, [n0, n1.astype(np.float32), n2], _images(rng, depths)


BACKFACING_BLOCK = (slice(20, 34), slice(40, 56))       # rows, columns of view 0


def _backfacing():
    from smvs_amd import synth
    main, subs = synth.ring_cameras(W, H, 2, flen=FLEN)
    cams = [main] + subs
    depths, normals = synth.depth_and_normal_maps(_scene(), cams)
    normals[0][BACKFACING_BLOCK] *= np.float32(-1.0)
    rng = np.random.default_rng(13)
    return cams, depths, normals, _images(rng, depths)


def _behind_camera():
    """Two ring views that agree, and between them in the list a camera beyond
    the scene that looks away from it at a wall of its own, half a unit away:
    every point of the ring views is behind it (proj[2] < 0), and its mirror
    image through the camera centre lands inside the view, on a pixel whose
    power is far above half the point's own.  Were the pair not skipped it
    would count as in front and be subtracted."""
    from smvs_amd import synth
    main, subs = synth.ring_cameras(W, H, 1, flen=FLEN)
    wall = synth.Camera(np.eye(3), -np.array([0.0, 0.0, 10.0]), 0.6, 64, 48)
    cams = [main, wall, subs[0]]
    depths, normals = synth.depth_and_normal_maps(_scene(), cams)
    depths[1][:] = 0.5
    normals[1][:] = (0.0, 0.0, 1.0)
    rng = np.random.default_rng(16)
    return cams, depths, normals, _images(rng, depths)


def _principal_plane():
    from smvs_amd import synth
    w, h = 64, 48
    cam0 = synth.Camera(np.eye(3), np.zeros(3), FLEN, w, h)
    d0, n0 = synth.depth_and_normal_maps(_scene(), [cam0])
    view0 = cut_ref.View(cam0, w, h)
    centres = []
    for x, y in PLANE_PIXELS:
        # world_point of csrc/mesh_shared.h in float, operation by operation
        centres.append(view0.world_point(np.array([x]), np.array([y]),
                                         d0[0][y:y + 1, x])[0].astype(np.float64))
    centres[1] = centres[1] + np.array([PLANE_SHIFT, 0.0, 0.0])
    # R = I, t = -centre: exact in float, the centres are float values
    cams = [cam0] + [synth.Camera(np.eye(3), -c, FLEN, w, h) for c in centres]
    cams.append(_camera((0.25, 0.05, 0.0), TARGET, w, h, FLEN))
    depths, normals = synth.depth_and_normal_maps(_scene(), cams)
    assert np.array_equal(depths[0], d0[0])
    # views 1 and 2 sit on the sphere's surface: they get a wall of their own,
    # five units away and facing them, instead of the sphere's inside
    for i in (1, 2):
        depths[i][:] = 5.0
        normals[i][:] = (0.0, 0.0, 1.0)
    # were (0, 0, 0) / 0 turned into pixel (0, 0) of view 1, that pixel would be
    # in front of the point with a power that outweighs the ring view's
    normals[1][0, 0] *= np.float32(1000.0)
    rng = np.random.default_rng(14)
    return cams, depths, normals, _images(rng, depths)


def _degenerate_sizes():
    from smvs_amd import synth
    main, subs = synth.ring_cameras(W, H, 1, flen=FLEN)
    cams = [main,
            _camera((0.1, -0.2, 0.0), TARGET, 2, 2, 0.8),
            _camera((-0.2, 0.1, 0.0), TARGET, 40, 30, 1.0),        # no depth at all
            _camera((0.3, 0.2, 0.1), TARGET, 1, 300, 1.2),
            subs[0]]
    depths, normals = synth.depth_and_normal_maps(_scene(), cams)
    depths[2][:] = 0.0
    rng = np.random.default_rng(15)
    for d in (depths[0], depths[4]):
        d *= (1.0 + 0.002 * rng.standard_normal(d.shape)).astype(np.float32)
    return cams, depths, normals, _images(rng, depths)


@functools.lru_cache(maxsize=None)
def get(name):
    if name == "mixed_wide_reversed":
        return Case(name, *[list(reversed(part)) for part in get("mixed_wide")[1:]])
    build = {"mixed_wide": _mixed_wide, "threshold_ladder": _threshold_ladder,
             "power_ladder": _power_ladder, "backfacing": _backfacing,
             "behind_camera": _behind_camera,
             "principal_plane": _principal_plane, "degenerate_sizes": _degenerate_sizes}[name]
    cams, depths, normals, images = build()
    depths = [np.ascontiguousarray(d, np.float32) for d in depths]
    normals = [np.ascontiguousarray(n, np.float32) for n in normals]
    return Case(name, cams, depths, normals, images)


_REFS = {}


def restated(name):
    """cut_ref.cut of a case, once per process (read-only)."""
    if name not in _REFS:
        c = get(name)
        _REFS[name] = cut_ref.cut(c.cams, c.depths, c.normals)
    return _REFS[name]


_ORACLE = {}


def oracle_cut(oracle, name):
    """oracle.cut_depth_maps of a case, once per process (read-only)."""
    if name not in _ORACLE:
        c = get(name)
        _ORACLE[name] = oracle.cut_depth_maps(c.cams, c.depths, c.normals)
    return _ORACLE[name]
