"""The brick cull's definition (the comment of smvs_tsdf_fuse_sparse_opts in
include/smvs_hip.h) restated in numpy on top of tests/tsdf_ref.py and tests/
tsdf_sparse_ref.py, which stay as they are: per view the min/max pyramid of the
prepared depth D, per brick the interval test against it.  Doubles, one
operation per operation of the definition, sums from left to right; the pyramid
is float32 min / max."""
import numpy as np

import tsdf_ref  # tests/tsdf_ref.py
import tsdf_sparse_ref  # tests/tsdf_sparse_ref.py

f32 = np.float32
BRICK = tsdf_sparse_ref.BRICK
EPS = 2.0 ** -21
TINY = 2.0 ** -140


def level0(D):
    """(lo, hi) of level 0: (D, D) where D < 0 or D > 0, else (+inf, -inf)"""
    D = np.asarray(D, f32)
    with np.errstate(invalid="ignore"):
        valid = (D < 0) | (D > 0)
    return (np.where(valid, D, f32(np.inf)).astype(f32),
            np.where(valid, D, f32(-np.inf)).astype(f32))


def pyramid(D):
    """-> [(lo, hi)] for the levels 0 .. (1 x 1); level l + 1 from level l"""
    lo, hi = level0(D)
    levels = [(lo, hi)]
    while lo.shape != (1, 1):
        h, w = lo.shape
        H, W = (h + 1) // 2, (w + 1) // 2
        plo = np.full((2 * H, 2 * W), np.inf, f32)
        phi = np.full((2 * H, 2 * W), -np.inf, f32)
        plo[:h, :w] = lo
        phi[:h, :w] = hi
        lo = plo.reshape(H, 2, W, 2).min(axis=(1, 3))
        hi = phi.reshape(H, 2, W, 2).max(axis=(1, 3))
        levels.append((lo, hi))
    return levels


def view_pyramids(cams, cut_maps):
    """per view: (V of tsdf_ref.camera, the pyramid of its prepared depth)"""
    out = []
    for cam, m in zip(cams, cut_maps):
        h, w = np.shape(m)
        V = tsdf_ref.camera(cam, w, h)
        out.append((V, pyramid(tsdf_ref.prepared_depth(V, m))))
    return out


def _axis_range(p_lo, p_hi, zs, zb, n):
    """the pixel range of one image axis where zlo > 0 -> first, last, outside"""
    ulo = np.minimum(p_lo / zs, p_lo / zb)
    uhi = np.maximum(p_hi / zs, p_hi / zb)
    ulo = np.minimum(np.maximum(ulo, -4.0), n + 4.0)
    uhi = np.minimum(np.maximum(uhi, -4.0), n + 4.0)
    first = np.floor(ulo).astype(np.int64) - 1
    last = np.floor(uhi).astype(np.int64) + 1
    outside = (last < 0) | (first > n - 1)
    return np.clip(first, 0, n - 1), np.clip(last, 0, n - 1), outside


def view_may_seed(V, levels, lo, hi, T):
    """one view against boxes [lo, hi] (three float64 arrays each) -> bool"""
    shape = lo[0].shape
    w, h = V["w"], V["h"]
    KR = [float(x) for x in V["KR"]]
    t = [float(x) for x in V["t"]]
    p_lo, p_hi = [], []
    for r in range(3):
        a = np.zeros(shape)
        b = np.zeros(shape)
        mag = np.full(shape, abs(t[r]))
        for k in range(3):
            m = KR[3 * r + k]
            p, q = m * lo[k], m * hi[k]
            a = a + np.minimum(p, q)
            b = b + np.maximum(p, q)
            mag = mag + abs(m) * np.maximum(np.abs(lo[k]), np.abs(hi[k]))
        e = EPS * mag + TINY
        p_lo.append((a - t[r]) - e)
        p_hi.append((b - t[r]) + e)
    finite = np.ones(shape, bool)
    for x in p_lo + p_hi:
        finite &= np.isfinite(x)
    zlo, zhi = p_lo[2], p_hi[2]
    with np.errstate(invalid="ignore"):
        behind = zhi <= 0
        proper = zlo > 0
    # (divisors of 1 where the quotient is not used)
    zs = np.where(proper & finite, zlo, 1.0)
    zb = np.where(proper & finite, zhi, 1.0)
    num = [np.where(finite, x, 0.0) for x in (p_lo[0], p_hi[0], p_lo[1], p_hi[1])]
    with np.errstate(over="ignore"):
        x0, x1, out_x = _axis_range(num[0], num[1], zs, zb, w)
        y0, y1, out_y = _axis_range(num[2], num[3], zs, zb, h)
    x0, x1 = np.where(proper, x0, 0), np.where(proper, x1, w - 1)
    y0, y1 = np.where(proper, y0, 0), np.where(proper, y1, h - 1)
    outside = proper & (out_x | out_y)
    level = np.zeros(shape, np.int64)
    for _ in range(len(levels)):
        level += ((x1 >> level) - (x0 >> level) > 1) | ((y1 >> level) - (y0 >> level) > 1)
    dlo = np.full(shape, np.inf, f32)
    dhi = np.full(shape, -np.inf, f32)
    for l, (plo, phi) in enumerate(levels):
        s = level == l
        if not s.any():
            continue
        for yy in (y0[s] >> l, y1[s] >> l):
            for xx in (x0[s] >> l, x1[s] >> l):
                dlo[s] = np.minimum(dlo[s], plo[yy, xx])
                dhi[s] = np.maximum(dhi[s], phi[yy, xx])
    with np.errstate(invalid="ignore"):
        near = (dhi.astype(np.float64) >= np.maximum(zlo, 0.0) - T) \
            & (dlo.astype(np.float64) <= zhi + T)
    may = ~behind & ~outside & (dlo <= dhi) & near
    return np.where(finite, may, True)


def brick_boxes(origin, voxel_size, dims, bz_range=None):
    """[lo, hi] per brick of the z-slabs bz_range of the brick grid, float64,
    each of shape (slabs, by, bx)"""
    vs = f32(voxel_size)
    bx, by, bz = tsdf_sparse_ref.brick_dims(dims)
    b0, b1 = (0, bz) if bz_range is None else bz_range
    count = (bx, by, b1 - b0)
    shape = count[::-1]
    lo, hi = [], []
    for a in range(3):
        c = tsdf_ref._centres(origin, vs, int(dims[a]), a).astype(np.float64)
        first = (np.arange(count[a]) + (b0 if a == 2 else 0)) * BRICK[a]
        last = np.minimum(first + BRICK[a] - 1, int(dims[a]) - 1)
        sl = [None, None, None]
        sl[2 - a] = slice(None)
        lo.append(np.broadcast_to(c[first][tuple(sl)], shape))
        hi.append(np.broadcast_to(c[last][tuple(sl)], shape))
    return lo, hi


def candidates(cams, cut_maps, origin, voxel_size, dims, trunc=0, bz_range=None, views=None):
    """brick_candidate of smvs_tsdf_fuse_sparse_opts on prepared (cut) maps ->
    (bz, by, bx) uint8, or the z-slabs bz_range = (first, end) of it.  views:
    view_pyramids(cams, cut_maps) computed before."""
    vs = f32(voxel_size)
    trunc = f32(trunc) if trunc > 0 else f32(3.0) * vs
    T = float(trunc) * (1.0 + 2.0 ** -22)
    lo, hi = brick_boxes(origin, voxel_size, dims, bz_range)
    if views is None:
        views = view_pyramids(cams, cut_maps)
    cand = np.zeros(lo[0].shape, bool)
    for V, levels in views:
        cand |= view_may_seed(V, levels, lo, hi, T)
    return cand.astype(np.uint8)


def pyramid_brute(D, level):
    """level `level` by the definition unrolled: the min / max over each texel's
    block of 2^level x 2^level pixels clipped to the image"""
    lo0, hi0 = level0(D)
    h, w = lo0.shape
    s = 1 << level
    H, W = -(-h // s), -(-w // s)
    lo = np.empty((H, W), f32)
    hi = np.empty((H, W), f32)
    for y in range(H):
        for x in range(W):
            lo[y, x] = lo0[y * s:(y + 1) * s, x * s:(x + 1) * s].min()
            hi[y, x] = hi0[y * s:(y + 1) * s, x * s:(x + 1) * s].max()
    return lo, hi


def fuse_on_candidates(cams, cut_maps, images, origin, voxel_size, dims, candidate, trunc=0,
                       min_weight=0):
    """tsdf_sparse_ref.fuse with the seed test run on the candidate bricks alone
    (the other bricks count as no seed) -> its dict, tested_bricks in stats"""
    dims = tuple(int(x) for x in dims)
    F, W, col = tsdf_ref.field(cams, cut_maps, images, origin, voxel_size, dims, trunc,
                               min_weight)
    bx, by, bz = tsdf_sparse_ref.brick_dims(dims)
    seeds = tsdf_sparse_ref._seed_bricks(col[..., 3], (bz, by, bx)) & (candidate != 0)
    state = tsdf_sparse_ref._state_of_seed_bricks(seeds)
    known = tsdf_sparse_ref._voxel_mask(state, F.shape)
    F = np.where(known, F, f32(np.nan)).astype(f32)
    W = np.where(known, W, 0).astype(np.uint32)
    col = np.where(known[..., None], col, 0).astype(np.uint32)
    dense = tsdf_ref.surface(F, W, col, origin, voxel_size, len(cams))
    idx, _ = tsdf_sparse_ref._active_cells(F)
    idx = tuple(x.astype(np.int64) for x in idx)
    out, _ = tsdf_sparse_ref.reorder(dense, idx, dims)
    out["brick_state"] = state
    allocated = int((state != 0).sum())
    out["stats"] = {"bricks": bx * by * bz, "seed_bricks": int((state == 2).sum()),
                    "allocated_bricks": allocated,
                    "state_bytes": allocated * tsdf_sparse_ref.STATE_BYTES_PER_BRICK,
                    "tested_bricks": int((candidate != 0).sum())}
    out["tsdf"] = F
    out["weight"] = W
    return out
