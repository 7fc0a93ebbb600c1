"""numpy restatement of the multi-view photo-consistency test of the SGM front
end (include/smvs_hip.h, "Multi-view photo-consistency test"; DESIGN.md section
3.6).

The sample is float32: every float operation is one np.float32 operation in the
written order, so there is nothing to contract and the divisions are IEEE's.
The sums are int64, the score and the mean float64.  Vectorised over the image:
one pass per witness and window offset."""
import numpy as np

F = np.float32


def sample(witness, M, t, xc, yc, depth):
    """(B, inside) of warped_neighbors_for_depth (lib/sgm_stereo.cc:163-188) for
    the main pixels (xc, yc) at `depth` (arrays of one shape), as the warp kernel
    of the runs evaluates it; inside stated positively, so a coordinate that is
    not a number is outside.  B is int64, 0 where outside."""
    witness = np.asarray(witness, np.uint8)
    nh, nw = witness.shape
    M = np.asarray(M, F).reshape(9)
    t = np.asarray(t, F).reshape(3)
    depth = np.asarray(depth, F)
    with np.errstate(all="ignore"):
        px = F(0.5) + np.asarray(xc).astype(F)
        py = F(0.5) + np.asarray(yc).astype(F)
        p = []
        for r in range(3):
            s = F(0.0) + M[3 * r + 0] * px
            s = s + M[3 * r + 1] * py
            s = s + M[3 * r + 2] * F(1.0)
            p.append(s * depth + t[r])
        p0, p1, p2 = p
        p0 = p0 / p2 - F(0.5)
        p1 = p1 / p2 - F(0.5)
        xmax, ymax = F(nw - 1), F(nh - 1)
        inside = ~(p2 < 0) & (p0 >= 0) & (p1 >= 0) & (p0 <= xmax) & (p1 <= ymax)
        # mve::Image<uint8_t>::linear_at
        fx = np.where(inside, np.maximum(F(0), np.minimum(xmax, p0)), F(0)).astype(F)
        fy = np.where(inside, np.maximum(F(0), np.minimum(ymax, p1)), F(0)).astype(F)
    ix, iy = fx.astype(np.int32), fy.astype(np.int32)
    ix1, iy1 = np.minimum(ix + 1, nw - 1), np.minimum(iy + 1, nh - 1)
    w1 = fx - ix.astype(F)
    w0 = F(1.0) - w1
    w3 = fy - iy.astype(F)
    w2 = F(1.0) - w3
    v1, v2 = witness[iy, ix].astype(F), witness[iy, ix1].astype(F)
    v3, v4 = witness[iy1, ix].astype(F), witness[iy1, ix1].astype(F)
    val = v1 * (w0 * w2) + v2 * (w1 * w2) + v3 * (w0 * w3) + v4 * (w1 * w3) + F(0.5)
    assert val.dtype == F
    # (uint8_t)(float): the conversion to an integer, then its low byte
    B = (val.astype(np.int32) & 0xFF).astype(np.int64)
    return np.where(inside, B, 0), inside


def window_sums(main_img, depth, witness, M, t, radius):
    """-> (SA, SB, SAB, SAA, SBB int64, defined) of every pixel's window against
    one witness at the pixel's own depth."""
    I = np.asarray(main_img, np.uint8)
    h, w = I.shape
    depth = np.asarray(depth, F)
    yy, xx = np.mgrid[0:h, 0:w]
    SA, SB, SAB, SAA, SBB = (np.zeros((h, w), np.int64) for _ in range(5))
    defined = np.ones((h, w), bool)
    for j in range(-radius, radius + 1):
        for i in range(-radius, radius + 1):
            xc = np.clip(xx + i, 0, w - 1)
            yc = np.clip(yy + j, 0, h - 1)
            A = I[yc, xc].astype(np.int64)
            B, inside = sample(witness, M, t, xc, yc, depth)
            defined &= inside
            SA += A
            SB += B
            SAB += A * B
            SAA += A * A
            SBB += B * B
    return SA, SB, SAB, SAA, SBB, defined


def witness_score(main_img, depth, witness, M, t, radius):
    """-> (score float64, defined): the signed squared correlation of every
    pixel's window with one witness; 0.0 for a flat window.  (What it holds where
    the witness is not defined means nothing.)"""
    N = (2 * radius + 1) ** 2
    SA, SB, SAB, SAA, SBB, defined = window_sums(main_img, depth, witness, M, t, radius)
    cov = N * SAB - SA * SB
    va = N * SAA - SA * SA
    vb = N * SBB - SB * SB
    flat = (va == 0) | (vb == 0)
    num = (cov * np.abs(cov)).astype(np.float64)
    den = np.where(flat, 1, va * vb).astype(np.float64)
    assert np.abs(cov * np.abs(cov))[defined].max(initial=0) < 2 ** 53 and (va * vb).max() < 2 ** 53
    return np.where(flat, 0.0, num / den), defined


def scores(main_img, depth, witnesses, radius):
    """-> (score (n, h, w) float64, defined (n, h, w)); witnesses: dicts {image,
    M_fwd, t_fwd}."""
    pairs = [witness_score(main_img, depth, nb["image"], nb["M_fwd"], nb["t_fwd"], radius)
             for nb in witnesses]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def fold(depth, score, defined, best_k, min_views, min_score):
    """The per-pixel part of the definition -> (out, confidence, views)."""
    depth = np.asarray(depth, F)
    n = score.shape[0]
    with np.errstate(invalid="ignore"):
        valid = depth > 0
    defined = defined & valid[None]
    c = defined.sum(axis=0)
    # the defined scores in descending order (the others behind them)
    ordered = -np.sort(-np.where(defined, score, -np.inf), axis=0)
    kk = np.minimum(best_k if best_k else n, c)
    total = np.zeros(depth.shape, np.float64)
    for s in range(n):
        total = np.where(s < kk, total + np.where(s < kk, ordered[s], 0.0), total)
    with np.errstate(all="ignore"):
        mean = (total / kk.astype(np.float64)).astype(F)
    conf = np.where(valid & (c >= max(min_views, 1)), mean, F(-1.0)).astype(F)
    out = depth.copy()
    out[valid & (conf < F(min_score))] = 0
    return out, conf, np.where(valid, c, 0).astype(np.uint8)


def photo_check(main_img, depth, witnesses, radius=2, best_k=2, min_views=2, min_score=0.49):
    """The whole test -> (out f32, confidence f32, views u8)."""
    score, defined = scores(main_img, depth, witnesses, radius)
    return fold(depth, score, defined, best_k, min_views, min_score)
