"""numpy restatement of the multi-view plane refinement sweeps of the SGM front
end (include/smvs_hip.h, "Multi-view plane refinement sweeps"; DESIGN.md section
3.6).

The sample and the per-pixel fold are those of tests/sgm_photo_ref.py; here the
depth is per window sample.  Every float operation is one np.float32 operation in
the written order, the hash is Python-exact uint32 arithmetic in uint64 arrays.
Vectorised per candidate over the active pixels of a half-sweep, which is
possible because a half-sweep only reads the other colour."""
import numpy as np

from sgm_photo_ref import sample, fold

F = np.float32
U = np.uint64
MASK = U(0xFFFFFFFF)

DEFAULTS = dict(sweeps=0, samples=2, depth_step=0.02, slant_step=0.01, seed=1, fill=1)


def mix(v):
    """mix of the definition on uint32 values held in uint64"""
    v = np.asarray(v, U) & MASK
    v = v ^ (v >> U(16))
    v = (v * U(0x7feb352d)) & MASK
    v = v ^ (v >> U(15))
    v = (v * U(0x846ca68b)) & MASK
    return v ^ (v >> U(16))


def units(seed, site, t, m):
    """(u_1, u_2, u_3) float32 of the pixels `site` = y * w + x"""
    h0 = mix(U(seed & 0xFFFFFFFF) ^ mix((np.asarray(site, U) & MASK) ^ mix(U(t * 16 + m))))
    out = []
    for j in (1, 2, 3):
        hj = mix((h0 + U(j * 0x9e3779b9)) & MASK)
        k = (hj >> U(8)).astype(np.int64) - 8388608
        out.append(k.astype(F) * F(2.0 ** -23))
    return out


def confidence(main_img, witnesses, photo, xs, ys, a, gx, gy):
    """-> (confidence f32, views u8) of the hypotheses (a, gx, gy), a > 0, at the
    pixels (xs, ys) (arrays of one shape); photo: (radius, best_k, min_views)."""
    radius, best_k, min_views = photo
    I = np.asarray(main_img, np.uint8)
    h, w = I.shape
    a, gx, gy = (np.asarray(v, F) for v in (a, gx, gy))
    N = (2 * radius + 1) ** 2
    score, defined = [], []
    # the window's depths and A, once
    taps = []
    with np.errstate(all="ignore"):
        for j in range(-radius, radius + 1):
            for i in range(-radius, radius + 1):
                xc = np.clip(xs + i, 0, w - 1)
                yc = np.clip(ys + j, 0, h - 1)
                d = a + gx * F(i)
                d = d + gy * F(j)
                assert d.dtype == F
                taps.append((xc, yc, I[yc, xc].astype(np.int64), d, d > 0))
    SA = sum(t[2] for t in taps)
    SAA = sum(t[2] * t[2] for t in taps)
    va = N * SAA - SA * SA
    for nb in witnesses:
        SB = np.zeros(a.shape, np.int64)
        SAB, SBB = SB.copy(), SB.copy()
        ok = np.ones(a.shape, bool)
        for xc, yc, A, d, pos in taps:
            B, inside = sample(nb["image"], nb["M_fwd"], nb["t_fwd"], xc, yc,
                               np.where(pos, d, F(1.0)))
            inside = inside & pos
            B = np.where(inside, B, 0)
            ok &= inside
            SB += B
            SAB += A * B
            SBB += B * B
        cov = N * SAB - SA * SB
        vb = N * SBB - SB * SB
        flat = (va == 0) | (vb == 0)
        num = (cov * np.abs(cov)).astype(np.float64)
        den = np.where(flat, 1, va * vb).astype(np.float64)
        score.append(np.where(flat, 0.0, num / den))
        defined.append(ok)
    _, conf, views = fold(a, np.stack(score), np.stack(defined), best_k, min_views, -1.0)
    return conf, views


def plane_refine(main_img, depth, witnesses, radius=2, best_k=2, min_views=2, min_score=0.49,
                 sweeps=0, samples=2, depth_step=0.02, slant_step=0.01, seed=1, fill=1,
                 counts=None):
    """The whole definition -> (out f32, slant f32 [h][w][2], confidence f32,
    views u8).  counts: a dict that receives the adoptions by propagation and by
    perturbation."""
    I = np.asarray(main_img, np.uint8)
    h, w = I.shape
    depth = np.asarray(depth, F)
    photo = (radius, best_k, min_views)
    depth_step, slant_step = F(depth_step), F(slant_step)
    a = np.zeros((h, w), F)
    gx, gy = a.copy(), a.copy()
    conf = np.full((h, w), -1.0, F)
    views = np.zeros((h, w), np.uint8)
    with np.errstate(invalid="ignore"):
        has = depth > 0
    yy, xx = np.mgrid[0:h, 0:w]
    ys, xs = yy[has], xx[has]
    a[has] = depth[has]
    if has.any():
        conf[has], views[has] = confidence(I, witnesses, photo, xs, ys, a[has], gx[has], gy[has])
    input_valid = has.copy()
    adopted = [0, 0]

    def consider(ys, xs, ok, na, ngx, ngy, kind):
        """the candidates (na, ngx, ngy) of the pixels (ys, xs) where ok"""
        ys, xs, na, ngx, ngy = ys[ok], xs[ok], na[ok], ngx[ok], ngy[ok]
        if ys.size == 0:
            return
        c, v = confidence(I, witnesses, photo, xs, ys, na, ngx, ngy)
        better = c > conf[ys, xs]
        ys, xs = ys[better], xs[better]
        a[ys, xs], gx[ys, xs], gy[ys, xs] = na[better], ngx[better], ngy[better]
        conf[ys, xs], views[ys, xs] = c[better], v[better]
        has[ys, xs] = True
        adopted[kind] += int(better.sum())

    for t in range(sweeps):
        s = F(2.0 ** -t)
        for c in (0, 1):
            active = ((xx + yy) & 1) == c
            if not fill:
                active &= input_valid
            ys, xs = yy[active], xx[active]
            for dx, dy in ((-1, 0), (1, 0), (0, -1), (0, 1)):
                xn, yn = xs + dx, ys + dy
                ok = (xn >= 0) & (xn < w) & (yn >= 0) & (yn < h)
                xn, yn = np.clip(xn, 0, w - 1), np.clip(yn, 0, h - 1)
                ok &= has[yn, xn]
                an, gxn, gyn = a[yn, xn], gx[yn, xn], gy[yn, xn]
                step = gxn if dy == 0 else gyn
                na = an + step if dx + dy < 0 else an - step
                assert na.dtype == F
                with np.errstate(invalid="ignore"):
                    ok &= na > 0
                consider(ys, xs, ok, na, gxn, gyn, 0)
            for m in range(samples):
                ok = has[ys, xs]
                ca, cgx, cgy = a[ys, xs], gx[ys, xs], gy[ys, xs]
                u1, u2, u3 = units(seed, ys * w + xs, t, m)
                with np.errstate(all="ignore"):
                    e = ca * depth_step
                    e = e * s
                    na = ca + e * u1
                    g = ca * slant_step
                    g = g * s
                    ngx = cgx + g * u2
                    ngy = cgy + g * u3
                    assert na.dtype == F and ngx.dtype == F and ngy.dtype == F
                    ok = ok & (na > 0)
                consider(ys, xs, ok, na, ngx, ngy, 1)
    out = depth.copy()
    out[has] = a[has]
    out[has & (conf < F(min_score))] = 0
    if counts is not None:
        counts["propagation"], counts["perturbation"] = adopted
    return out, np.stack([gx, gy], axis=-1), conf, views
