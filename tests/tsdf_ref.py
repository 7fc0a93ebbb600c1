"""The definition of the volumetric fusion (the comment of smvs_tsdf_fuse in
include/smvs_hip.h) restated in numpy float32: vectorised, one numpy operation
per float operation of the definition, so that it rounds as the device does.

Its inputs are the PREPARED maps: the cut maps (ray length, 0 = cut or hole) as
oracle.cut_depth_maps returns them, or the depth maps themselves where nothing
is cut.  D, the z-depth the field reads, follows from them alone: it is the
prepared z-depth where the cut map is non-zero, and the cut map holds the input
depth there."""
import numpy as np

f32 = np.float32

EDGES = [(0, 1, 0), (2, 3, 0), (4, 5, 0), (6, 7, 0),
         (0, 2, 1), (1, 3, 1), (4, 6, 1), (5, 7, 1),
         (0, 4, 2), (1, 5, 2), (2, 6, 2), (3, 7, 2)]


def camera(cam, w, h):
    """fill_view_camera of csrc/mesh_cut.hip: invproj, KR, t, rot, c2w_t (float32,
    its summation order)."""
    flen, fw, fh = f32(cam.flen), f32(w), f32(h)
    ax = flen * max(fw, fh)
    z, one, half = f32(0), f32(1), f32(0.5)
    K = [ax, z, fw * half, z, ax, fh * half, z, z, one]
    Ki = [one / ax, z, -fw * half / ax, z, one / ax, -fh * half / ax, z, z, one]
    rot = [f32(x) for x in np.asarray(cam.R, f32).reshape(9)]
    trans = [f32(x) for x in np.asarray(cam.t, f32).reshape(3)]
    KR = []
    for r in range(3):
        for c in range(3):
            s = f32(0)
            for k in range(3):
                s = s + K[3 * r + k] * rot[3 * k + c]
            KR.append(s)
    pos = []
    for r in range(3):
        s = f32(0)
        for k in range(3):
            s = s + (-rot[3 * k + r]) * trans[k]
        pos.append(s)
    t = []
    for r in range(3):
        s = f32(0)
        for k in range(3):
            s = s + KR[3 * r + k] * pos[k]
        t.append(s)
    return dict(w=w, h=h, invproj=Ki, KR=KR, t=t, rot=rot, c2w_t=pos)


def _pixel_rays(V):
    """invproj * (x + .5, y + .5, 1) per pixel and its length (world_point)"""
    h, w = V["h"], V["w"]
    px = (np.arange(w, dtype=f32) + f32(0.5))[None, :]
    py = (np.arange(h, dtype=f32) + f32(0.5))[:, None]
    v = []
    for r in range(3):
        s = f32(0) + V["invproj"][3 * r] * px
        s = s + V["invproj"][3 * r + 1] * py
        s = s + V["invproj"][3 * r + 2] * f32(1)
        v.append(np.broadcast_to(s, (h, w)).astype(f32))
    length = np.sqrt(((f32(0) + v[0] * v[0]) + v[1] * v[1]) + v[2] * v[2])
    return v, length


def prepared_depth(V, cut_map):
    """D: mesh_prepare_kernel's z-depth of the pixels the cut keeps, else 0"""
    _, length = _pixel_rays(V)
    d = np.asarray(cut_map, f32)
    dz = (d.astype(np.float64) * (1.0 / length.astype(np.float64))).astype(f32)
    return np.where(d != 0, dz, f32(0)).astype(f32)


def world_points(V, cut_map):
    """world_point of every valid pixel of the map -> (n, 3)"""
    v, length = _pixel_rays(V)
    d = np.asarray(cut_map, f32)
    pc = [v[r] / length * d for r in range(3)]
    pos = []
    for r in range(3):
        s = f32(0) + V["rot"][r] * pc[0]
        s = s + V["rot"][3 + r] * pc[1]
        s = s + V["rot"][6 + r] * pc[2]
        pos.append(s + V["c2w_t"][r] * f32(1))
    return np.stack(pos, -1)[d != 0]


def bounds(cams, cut_maps):
    """smvs_tsdf_bounds: (lo, hi); (+inf, -inf) without a valid pixel"""
    lo = np.full(3, np.inf, f32)
    hi = np.full(3, -np.inf, f32)
    for cam, d in zip(cams, cut_maps):
        h, w = d.shape
        p = world_points(camera(cam, w, h), d)
        if len(p):
            lo = np.minimum(lo, p.min(axis=0))
            hi = np.maximum(hi, p.max(axis=0))
    return lo, hi


def _centres(origin, voxel_size, n, axis):
    return f32(origin[axis]) + (np.arange(n, dtype=f32) + f32(0.5)) * f32(voxel_size)


def field(cams, cut_maps, images, origin, voxel_size, dims, trunc=0, min_weight=0):
    """Field, steps 1-8 -> F (nz, ny, nx) float32 with NaN = unknown, W uint32,
    colour sums (nz, ny, nx, 4) uint32 (R, G, B, C)"""
    nx, ny, nz = (int(x) for x in dims)
    vs = f32(voxel_size)
    trunc = f32(trunc) if trunc > 0 else f32(3.0) * vs
    min_weight = int(min_weight) if min_weight > 0 else 1
    shape = (nz, ny, nx)
    cx = np.broadcast_to(_centres(origin, vs, nx, 0)[None, None, :], shape)
    cy = np.broadcast_to(_centres(origin, vs, ny, 1)[None, :, None], shape)
    cz = np.broadcast_to(_centres(origin, vs, nz, 2)[:, None, None], shape)
    S = np.zeros(shape, f32)
    W = np.zeros(shape, np.uint32)
    col = np.zeros(shape + (4,), np.uint32)
    for cam, cut_map, image in zip(cams, cut_maps, images):
        h, w = cut_map.shape
        V = camera(cam, w, h)
        D = prepared_depth(V, cut_map)
        img = np.asarray(image, np.uint8).reshape(h, w, -1)
        KR, t = V["KR"], V["t"]
        proj = []
        for r in range(3):
            s = f32(0) + KR[3 * r] * cx
            s = s + KR[3 * r + 1] * cy
            s = s + KR[3 * r + 2] * cz
            proj.append(s - t[r])
        ok = ~(proj[2] <= 0)
        den = np.where(ok, proj[2], f32(1))
        u = proj[0] / den
        v = proj[1] / den
        ok &= ~((u < 0) | (v < 0))
        # (int)u >= w exactly when u >= w for u >= 0: decided before the cast
        ok &= ~((u >= f32(w)) | (v >= f32(h)))
        xj = np.where(ok, u, f32(0)).astype(np.int32)
        yj = np.where(ok, v, f32(0)).astype(np.int32)
        d = D[yj, xj]
        ok &= ~(d == 0)
        sdf = d - proj[2]
        ok &= ~(sdf < -trunc)
        S = np.where(ok, S + np.fmin(f32(1), sdf / trunc), S)
        W = W + ok.astype(np.uint32)
        near = ok & (sdf <= trunc)
        px = img[yj, xj]
        rgb = px[..., :3] if px.shape[-1] >= 3 else np.repeat(px[..., :1], 3, axis=-1)
        col[..., :3] += np.where(near[..., None], rgb, 0).astype(np.uint32)
        col[..., 3] += near.astype(np.uint32)
    with np.errstate(invalid="ignore", divide="ignore"):
        F = np.where(W >= min_weight, S / W.astype(f32), f32(np.nan)).astype(f32)
    return F, W, col


def _corner(a, c):
    """the cells' view of corner c = dx + 2 dy + 4 dz of a point array"""
    nz, ny, nx = a.shape[:3]
    dx, dy, dz = c & 1, c >> 1 & 1, c >> 2
    return a[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]


def _at_offset(cells, point_shape, off_xyz, fill):
    """cells (nz-1, ny-1, nx-1, ...) -> point-shaped array whose entry P is
    cells[P + off] (off per xyz axis, 0 or -1), `fill` where that is no cell"""
    out = np.full(point_shape + cells.shape[3:], fill, cells.dtype)
    dst, src = [], []
    for axis in (2, 1, 0):       # numpy axes z, y, x <- xyz axes 2, 1, 0
        n = cells.shape[2 - axis]
        if off_xyz[axis] == 0:
            dst.append(slice(0, n))
            src.append(slice(0, n))
        else:
            dst.append(slice(1, n + 1))
            src.append(slice(0, n))
    out[tuple(dst)] = cells[tuple(src)]
    return out


def surface(F, W, col, origin, voxel_size, n_views):
    """Vertices and faces of the field -> dict xyz, normals, rgb, confidence,
    faces"""
    vs = f32(voxel_size)
    nz, ny, nx = F.shape
    f = np.stack([_corner(F, c) for c in range(8)], -1)
    complete = ~np.isnan(f).any(axis=-1)
    with np.errstate(invalid="ignore"):
        n_in = (f < 0).sum(axis=-1)
    active = complete & (n_in != 0) & (n_in != 8)
    kk, jj, ii = np.nonzero(active)          # C order: the linear cell index
    idx = [ii, jj, kk]
    fa_ = f[active]
    n = len(ii)
    total = [np.zeros(n, f32) for _ in range(3)]
    g = [np.zeros(n, f32) for _ in range(3)]
    m = np.zeros(n, np.int32)
    for a, b, axis in EDGES:
        Fa, Fb = fa_[:, a], fa_[:, b]
        g[axis] = g[axis] + (Fb - Fa)
        cross = (Fa < 0) != (Fb < 0)
        with np.errstate(invalid="ignore", divide="ignore"):
            t = Fa / (Fa - Fb)
        q = [f32(origin[r]) + ((idx[r] + (a >> r & 1)).astype(f32) + f32(0.5)) * vs
             for r in range(3)]
        with np.errstate(invalid="ignore"):
            q[axis] = q[axis] + t * vs
        for r in range(3):
            total[r] = np.where(cross, total[r] + q[r], total[r])
        m += cross
    xyz = np.stack([total[r] / m.astype(f32) for r in range(3)], -1).astype(f32)
    length = np.sqrt(((f32(0) + g[0] * g[0]) + g[1] * g[1]) + g[2] * g[2])
    with np.errstate(invalid="ignore", divide="ignore"):
        nrm = np.stack([np.where(length == 0, f32(0), g[r] / length) for r in range(3)], -1)
    sums = sum(_corner(col, c)[active].astype(np.uint32) for c in range(8)) \
        if n else np.zeros((0, 4), np.uint32)
    Cs = sums[:, 3:4]
    rgb = np.where(Cs == 0, 0, (2 * sums[:, :3] + Cs) // np.maximum(2 * Cs, 1)).astype(np.uint8)
    Ws = sum(_corner(W, c)[active].astype(np.uint32) for c in range(8)) \
        if n else np.zeros(0, np.uint32)
    conf = Ws.astype(f32) / f32(8 * n_views)

    vid_cells = np.full(active.shape, -1, np.int64)
    vid_cells[active] = np.arange(n)
    shape = F.shape
    lin = np.arange(F.size, dtype=np.int64).reshape(shape)
    known = ~np.isnan(F)
    with np.errstate(invalid="ignore"):
        inside = known & (F < 0)
    keys, tris = [], []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        npa = 2 - a
        # the far end P + e_a (no quad on the last layer along a)
        far_known = np.zeros(shape, bool)
        far_inside = np.zeros(shape, bool)
        sl_dst = [slice(None)] * 3
        sl_src = [slice(None)] * 3
        sl_dst[npa] = slice(0, shape[npa] - 1)
        sl_src[npa] = slice(1, shape[npa])
        far_known[tuple(sl_dst)] = known[tuple(sl_src)]
        far_inside[tuple(sl_dst)] = inside[tuple(sl_src)]
        quad = known & far_known & (inside != far_inside)
        v = []
        for ob, oc in ((-1, -1), (0, -1), (0, 0), (-1, 0)):
            off = [0, 0, 0]
            off[b], off[c] = ob, oc
            quad &= _at_offset(complete, shape, off, False)
            v.append(_at_offset(vid_cells, shape, off, -1))
        at = np.nonzero(quad.reshape(-1))[0]
        v = [x.reshape(-1)[at] for x in v]
        ins = inside.reshape(-1)[at]
        first = np.stack([v[0], np.where(ins, v[1], v[2]), np.where(ins, v[2], v[1])], -1)
        second = np.stack([v[0], np.where(ins, v[2], v[3]), np.where(ins, v[3], v[2])], -1)
        keys.append(lin.reshape(-1)[at] * 3 + a)
        tris.append(np.stack([first, second], 1))
    keys = np.concatenate(keys)
    tris = np.concatenate(tris) if len(keys) else np.zeros((0, 2, 3), np.int64)
    order = np.argsort(keys, kind="stable")
    faces = tris[order].reshape(-1, 3)
    assert faces.size == 0 or faces.min() >= 0
    return {"xyz": xyz, "normals": nrm.astype(f32), "rgb": rgb, "confidence": conf.astype(f32),
            "faces": faces.astype(np.uint32)}


def fuse(cams, cut_maps, images, origin, voxel_size, dims, trunc=0, min_weight=0):
    """smvs_tsdf_fuse on prepared maps -> the mesh dict plus tsdf and weight"""
    F, W, col = field(cams, cut_maps, images, origin, voxel_size, dims, trunc, min_weight)
    out = surface(F, W, col, origin, voxel_size, len(cams))
    out["tsdf"] = F
    out["weight"] = W
    return out
