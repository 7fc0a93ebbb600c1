"""MeshGenerator::cut_depth_maps (lib/mesh_generator.cc:24-158) with the normal
preparation of generate_mesh (:189-208) and ViewProjection (:300-342), restated
in float32 numpy with a label on every decision -- a second reading next to
oracle/smvs_oracle_front.c, vectorised over the pixels of view i for one other
view j at a time.  No GPU, no oracle: plain numpy.

Every product is rounded to float32 before it is added, sums run left to right
from 0.0f, division and sqrt are numpy's correctly rounded float32 ones, the
four threshold comparisons widen their float operands to float64, and the
conversion of the projected quotient to int is written out: truncation toward
zero of a finite quotient that fits an int32; any other quotient skips the pair
(what `static_cast<int>` gives on x86: INT_MIN, which is < 0).

cut() returns, next to the cut maps and world normals, per view i

  outcome  (n_views, h, w) uint8: what view j did to the pixel (NONE for
           j == i and for pixels without depth), evaluated for every j whether
           or not the pixel's walk had ended
  stopped  (n_views, h, w) bool: the walk had ended at a `break` before j
  reason   (h, w) uint8: why the pixel was cut, or KEPT
  power    (h, w) float32: the pixel's own surface power
  sum      (h, w) float32: the consistency sum at the end of the walk
  proj, quot, dm_j, power_j, power_jj   per (j, pixel): the operands of the
           decisions (NaN where the pair did not get that far)
"""
import numpy as np

f32 = np.float32

# per (pixel, other view)
(NONE, BEHIND, OUTSIDE, HOLE, OCCLUDED, FRONT_SUB, FRONT_IGNORED, BREAK, ADD) = range(9)
OUTCOMES = ("none", "behind", "outside", "hole", "occluded", "front_sub", "front_ignored",
            "break", "add")
# per pixel
(NO_DEPTH, BACKFACING, BROKE, SUM_NEGATIVE, SUM_ZERO, KEPT) = range(6)
REASONS = ("no_depth", "backfacing", "break", "sum_negative", "sum_zero", "kept")


def _dot3(a, b):
    """s = 0; s += a[0] * b[0]; s += a[1] * b[1]; s += a[2] * b[2] on the last
    axis, every product and sum rounded to float32."""
    s = np.zeros(np.broadcast(a[..., 0], b[..., 0]).shape, f32)
    for k in range(3):
        s = s + a[..., k] * b[..., k]
    return s


class View:
    """CameraInfo::fill_calibration / fill_inverse_calibration at the depth
    map's size, ViewProjection's KR and t, the cam-to-world translation."""

    def __init__(self, cam, w, h):
        self.w, self.h = int(w), int(h)
        flen = f32(cam.flen)
        fw, fh = f32(w), f32(h)
        ax = flen * f32(max(w, h))
        zero, one, half = f32(0), f32(1), f32(0.5)
        self.K = np.array([[ax, zero, fw * half], [zero, ax, fh * half], [zero, zero, one]], f32)
        self.invproj = np.array([[one / ax, zero, -fw * half / ax],
                                 [zero, one / ax, -fh * half / ax], [zero, zero, one]], f32)
        self.rot = np.asarray(cam.R, f32).reshape(3, 3)
        trans = np.asarray(cam.t, f32).reshape(3)
        self.KR = np.zeros((3, 3), f32)
        for r in range(3):
            for c in range(3):
                s = f32(0)
                for k in range(3):
                    s = f32(s + f32(self.K[r, k] * self.rot[k, c]))
                self.KR[r, c] = s
        # fill_camera_pos = the translation of fill_cam_to_world: -R^T t
        self.c2w_t = np.zeros(3, f32)
        for r in range(3):
            s = f32(0)
            for k in range(3):
                s = f32(s + f32(-self.rot[k, r] * trans[k]))
            self.c2w_t[r] = s
        self.t = np.zeros(3, f32)
        for r in range(3):
            s = f32(0)
            for k in range(3):
                s = f32(s + f32(self.KR[r, k] * self.c2w_t[k]))
            self.t[r] = s

    def rays(self, x, y):
        """invproj * (x + 0.5, y + 0.5, 1) and its length."""
        px = x.astype(f32) + f32(0.5)
        py = y.astype(f32) + f32(0.5)
        v = np.zeros(px.shape + (3,), f32)
        for r in range(3):
            s = np.zeros(px.shape, f32)
            s = s + self.invproj[r, 0] * px
            s = s + self.invproj[r, 1] * py
            s = s + self.invproj[r, 2] * f32(1)
            v[..., r] = s
        return v, np.sqrt(_dot3(v, v))

    def world_point(self, x, y, depth):
        """mve::geom::pixel_3dpos, then Matrix4f::mult(pos, 1) with the
        cam-to-world matrix (:80-82, :120-123)."""
        v, length = self.rays(x, y)
        pc = v / length[..., None] * depth[..., None]
        pos = np.zeros_like(pc)
        for r in range(3):
            s = np.zeros(depth.shape, f32)
            for k in range(3):
                s = s + self.rot[k, r] * pc[..., k]
            pos[..., r] = s + self.c2w_t[r] * f32(1)
        return pos

    def world_normals(self, normals):
        """:197-208: rot^T * (n0, -n1, -n2)."""
        n = np.stack([normals[..., 0], -normals[..., 1], -normals[..., 2]], -1).astype(f32)
        out = np.zeros_like(n)
        for r in range(3):
            s = np.zeros(n.shape[:-1], f32)
            for k in range(3):
                s = s + self.rot[k, r] * n[..., k]
            out[..., r] = s
        return out

    def z_depth(self, depth):
        """depthmap_convert_conventions(dm, invproj, false): `double len =
        px.norm(); dm *= 1.0 / len` with a float norm."""
        y, x = np.mgrid[0:self.h, 0:self.w]
        _, length = self.rays(x, y)
        return (depth.astype(np.float64) * (1.0 / length.astype(np.float64))).astype(f32)

    def proj(self, pos):
        """ViewProjection::get_proj."""
        return np.stack([_dot3(self.KR[r], pos) - self.t[r] for r in range(3)], -1)

    def surface_power(self, pos, normal):
        """ViewProjection::get_surface_power."""
        u, v, w = (_dot3(self.KR[r], pos) - self.t[r] for r in range(3))
        denom = w * w
        with np.errstate(all="ignore"):
            u_dx = np.stack([(self.KR[0, k] * w - self.KR[2, k] * u) / denom
                             for k in range(3)], -1)
            v_dx = np.stack([(self.KR[1, k] * w - self.KR[2, k] * v) / denom
                             for k in range(3)], -1)
            cr = np.stack([u_dx[..., 1] * v_dx[..., 2] - u_dx[..., 2] * v_dx[..., 1],
                           u_dx[..., 2] * v_dx[..., 0] - u_dx[..., 0] * v_dx[..., 2],
                           u_dx[..., 0] * v_dx[..., 1] - u_dx[..., 1] * v_dx[..., 0]], -1)
            return -_dot3(normal, cr)


def to_int(q):
    """static_cast<int>(float) as the reference's x86 build behaves: (fits,
    value) -- truncation toward zero where the quotient is finite and inside
    [-2^31, 2^31); anything else counts as a negative coordinate."""
    with np.errstate(invalid="ignore"):
        fits = np.isfinite(q) & (q >= f32(-2147483648.0)) & (q < f32(2147483648.0))
    value = np.where(fits, np.trunc(np.where(fits, q, 0)), -1).astype(np.int64)
    return fits, value


def compare(dm_j, z, power, power_j, power_jj, dtype=np.float64):
    """The four threshold tests of :128-138 with their operands widened to
    `dtype` (the reference: float64; float32 is what a kernel that compared in
    float would do, for the sensitivity count of test_cut_cases_cpu.py):
    -> (occluded, in_front, subtract, break by power_jj, break by power_j)."""
    c = lambda a: a.astype(dtype)  # noqa: E731
    with np.errstate(all="ignore"):
        occluded = c(dm_j) * dtype(1.01) < c(z)
        in_front = c(dm_j) * dtype(0.997) > c(z)
        subtract = c(power_jj) > dtype(0.5) * c(power)
        brk_jj = c(power_jj) > dtype(2.0) * c(power)
        brk_j = c(power_j) > dtype(2.0) * c(power)
    return occluded, in_front, subtract, brk_jj, brk_j


def classify(occluded, in_front, subtract, brk_jj, brk_j):
    """The outcome of a pair that reached the threshold tests."""
    return np.where(occluded, OCCLUDED,
                    np.where(in_front, np.where(subtract, FRONT_SUB, FRONT_IGNORED),
                             np.where(brk_jj | brk_j, BREAK, ADD))).astype(np.uint8)


VARIANTS = (None, "float_compare", "floorf", "no_behind_test")


def cut(cams, depths, normals, variant=None):
    """-> (cut maps, world normals, info); info[i] is the dict of the module's
    docstring for view i.

    variant: None is the reference.  The others are what a subtly wrong kernel
    would compute -- the thresholds compared in float, floorf in place of the
    truncation, the `proj[2] < 0` test dropped -- so that the CPU test can
    count the pixels of each case that such a kernel would get wrong."""
    assert variant in VARIANTS
    dtype = np.float32 if variant == "float_compare" else np.float64
    n = len(cams)
    depths = [np.ascontiguousarray(d, f32) for d in depths]
    views = [View(c, d.shape[1], d.shape[0]) for c, d in zip(cams, depths)]
    wn = [v.world_normals(np.asarray(m, f32)) for v, m in zip(views, normals)]
    cuts = [d.copy() for d in depths]
    if n < 2:     # a single depth map is returned unchanged (:208)
        return cuts, wn, [None] * n
    dz = [v.z_depth(d) for v, d in zip(views, depths)]
    infos = []
    for i in range(n):
        V, d = views[i], depths[i]
        h, w = d.shape
        ys, xs = np.nonzero(d != 0)
        m = len(ys)
        pos = V.world_point(xs, ys, d[ys, xs])
        normal = wn[i][ys, xs]
        power = V.surface_power(pos, normal)
        consistency = np.zeros(m, f32)
        stopped = np.zeros(m, bool)
        outcome = np.zeros((n, m), np.uint8)
        was_stopped = np.zeros((n, m), bool)
        nan = lambda *s: np.full(s, np.nan, f32)  # noqa: E731
        rec = dict(proj=nan(n, m, 3), quot=nan(n, m, 2), dm_j=nan(n, m), power_j=nan(n, m),
                   power_jj=nan(n, m))
        for j in range(n):
            if j == i:
                continue
            N = views[j]
            was_stopped[j] = stopped
            proj = N.proj(pos)
            rec["proj"][j] = proj
            out = np.full(m, NONE, np.uint8)
            with np.errstate(invalid="ignore"):
                behind = proj[:, 2] < 0
            if variant == "no_behind_test":
                behind[:] = False
            out[behind] = BEHIND
            with np.errstate(all="ignore"):
                qx = proj[:, 0] / proj[:, 2]
                qy = proj[:, 1] / proj[:, 2]
            rec["quot"][j] = np.where(behind[:, None], np.nan, np.stack([qx, qy], -1))
            if variant == "floorf":
                with np.errstate(invalid="ignore"):
                    qx, qy = np.floor(qx), np.floor(qy)
            fx, xj = to_int(qx)
            fy, yj = to_int(qy)
            inside = fx & fy & (xj >= 0) & (xj < N.w) & (yj >= 0) & (yj < N.h)
            out[~behind & ~inside] = OUTSIDE
            a = np.nonzero(~behind & inside)[0]
            dm_j = dz[j][yj[a], xj[a]]
            out[a[dm_j == 0]] = HOLE
            a, dm_j = a[dm_j != 0], dm_j[dm_j != 0]
            xa, ya = xj[a], yj[a]
            power_j = N.surface_power(pos[a], normal[a])
            pos_j = N.world_point(xa, ya, depths[j][ya, xa])
            power_jj = N.surface_power(pos_j, wn[j][ya, xa])
            rec["dm_j"][j, a], rec["power_j"][j, a], rec["power_jj"][j, a] = (
                dm_j, power_j, power_jj)
            o = classify(*compare(dm_j, proj[a, 2], power[a], power_j, power_jj, dtype=dtype))
            out[a] = o
            outcome[j] = out
            live = ~stopped[a]
            with np.errstate(all="ignore"):
                sub = a[live & (o == FRONT_SUB)]
                consistency[sub] = consistency[sub] - power_jj[live & (o == FRONT_SUB)]
                add = a[live & (o == ADD)]
                consistency[add] = consistency[add] + power_jj[live & (o == ADD)]
            stopped[a[live & (o == BREAK)]] = True
        with np.errstate(invalid="ignore"):
            reason = np.where(power < 0, BACKFACING,
                              np.where(stopped, BROKE,
                                       np.where(consistency < 0, SUM_NEGATIVE,
                                                np.where(consistency == 0, SUM_ZERO, KEPT))))
            is_cut = (power < 0) | stopped | (consistency <= 0)
        cuts[i][ys[is_cut], xs[is_cut]] = 0.0

        def full(a, fill, dtype):
            o = np.full(a.shape[:-1] + (h, w), fill, dtype) if a.ndim > 1 else \
                np.full((h, w), fill, dtype)
            o[..., ys, xs] = a
            return o
        info = dict(outcome=full(outcome, NONE, np.uint8),
                    stopped=full(was_stopped, False, bool),
                    reason=full(reason.astype(np.uint8), NO_DEPTH, np.uint8),
                    power=full(power, np.nan, f32), sum=full(consistency, np.nan, f32),
                    pixels=(ys, xs), view=V)
        info.update(rec)        # per (j, valid pixel), in the order of `pixels`
        info["outcome_px"], info["stopped_px"] = outcome, was_stopped
        infos.append(info)
    return cuts, wn, infos


def describe(info, y, x):
    """The restatement's walk of pixel (x, y) as text, for a failure message."""
    names = []
    for j in range(info["outcome"].shape[0]):
        o = info["outcome"][j, y, x]
        if o != NONE:
            names.append("%d:%s%s" % (j, OUTCOMES[o], "(after break)" if info["stopped"][j, y, x]
                                      else ""))
    return "reason %s, power %r, sum %r, views %s" % (
        REASONS[info["reason"][y, x]], info["power"][y, x], info["sum"][y, x], " ".join(names))
