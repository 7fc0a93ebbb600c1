"""A numpy restatement of the consensus merge of the SGM front end
(SMVS_SGM_MERGE_CONSENSUS, include/smvs_hip.h): float32
operations in the order of the definition, one candidate k at a time.

    best = 0, best_count = 0
    for k = 0 .. n-1 with c[k] != 0:
        count = number of j with c[j] != 0 and
                (j == k  or  fminf(c[j], c[k]) / fmaxf(c[j], c[k]) >= agree_ratio)
        if count > best_count: best_count = count, best = k
    if best_count == 0 or best_count < min_agree: out = 0
    else: s = 0.0f; for j ascending over the supporters of c[best]: s = s + c[j]
          out = s / (float)best_count
"""
import numpy as np

F = np.float32


def stars(stack, agree_ratio):
    """-> bool (n, n, ...): [k, j] is set where c[j] supports the candidate c[k]
    (both non-zero; j == k, or the ratio of the smaller to the larger of the two
    is at least agree_ratio, divided in float32)."""
    c = np.asarray(stack, F)
    n = c.shape[0]
    r = F(agree_ratio)
    out = np.zeros((n, n) + c.shape[1:], bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in range(n):
            for j in range(n):
                both = (c[k] != 0) & (c[j] != 0)
                if j == k:
                    out[k, j] = both
                    continue
                ratio = (np.minimum(c[j], c[k]) / np.maximum(c[j], c[k])).astype(F)
                out[k, j] = both & (ratio >= r)
    return out


def consensus(stack, agree_ratio, min_agree):
    """stack (n, ...) float32 checked depths, 0 = none
    -> (merged float32, support uint8, best int32: the winning candidate, 0
    where there is none)."""
    c = np.asarray(stack, F)
    assert c.dtype == F and c.ndim >= 1
    n = c.shape[0]
    star = stars(c, agree_ratio)
    best = np.zeros(c.shape[1:], np.int32)
    best_count = np.zeros(c.shape[1:], np.int32)
    for k in range(n):
        count = star[k].sum(axis=0).astype(np.int32)
        better = count > best_count               # strict: ties keep the lowest k
        best = np.where(better, k, best).astype(np.int32)
        best_count = np.where(better, count, best_count).astype(np.int32)
    s = np.zeros(c.shape[1:], F)
    for j in range(n):
        mine = np.take_along_axis(star[:, j], best[None], axis=0)[0]
        s = np.where(mine, (s + c[j]).astype(F), s).astype(F)
    keep = (best_count != 0) & (best_count >= int(min_agree))
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = (s / best_count.astype(F)).astype(F)
    merged = np.where(keep, mean, F(0)).astype(F)
    return merged, best_count.astype(np.uint8), best


def reference_merge(first, second):
    """app/smvsrecon.cc:366-377: the second map where the first has none, the
    mean where both have a depth"""
    first, second = np.asarray(first, F), np.asarray(second, F)
    return np.where(second == 0, first,
                    np.where(first == 0, second, (first + second) * F(0.5))).astype(F)


def lr_check_branches(fwd, bwd, M, t):
    """Which way each pixel of one left/right check goes (sgm_stereo.cc:64-91,
    the arithmetic of the oracle's check restated in float64 / float32):
    -> dict of bool maps: no_depth, border, zero_neighbor, ratio, kept."""
    fwd = np.asarray(fwd, F)
    bwd = np.asarray(bwd, F)
    M = np.asarray(M, F).reshape(9).astype(np.float64)
    t = np.asarray(t, F).reshape(3).astype(np.float64)
    h, w = fwd.shape
    nh, nw = bwd.shape
    cut = int(0.03 * float(max(nw, nh)))
    v, u = np.mgrid[0:h, 0:w].astype(np.float64)
    wd = fwd.astype(np.float64)
    p = M[0] * u + M[1] * v + M[2]
    q = M[3] * u + M[4] * v + M[5]
    r = M[6] * u + M[7] * v + M[8]
    a, b, d = wd * p + t[0], wd * q + t[1], wd * r + t[2]
    with np.errstate(divide="ignore", invalid="ignore"):
        cx, cy = a / d, b / d
    has = fwd != 0
    inside = (cx >= cut) & (cx < nw - cut) & (cy >= cut) & (cy < nh - cut)
    ix = np.where(inside, cx, 0).astype(np.int64)
    iy = np.where(inside, cy, 0).astype(np.int64)
    nd = bwd[iy, ix]
    cd = d.astype(F)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = (np.minimum(cd, nd) / np.maximum(cd, nd)).astype(F)
    zero = has & inside & (nd == 0)
    low = has & inside & (nd != 0) & (ratio.astype(np.float64) < 0.8)
    return dict(no_depth=~has, border=has & ~inside, zero_neighbor=zero, ratio=low,
                kept=has & inside & ~zero & ~low)
