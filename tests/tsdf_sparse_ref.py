"""The brick-sparse fusion's definition (the comment of smvs_tsdf_fuse_sparse in
include/smvs_hip.h) restated on top of tests/tsdf_ref.py, which stays as it is:
the dense field, masked to the allocated bricks, through the dense surface
rules, then vertices and faces permuted into the sparse order.  For grids the
dense restatement cannot hold, field_window restates steps 1-8 on an index
window of the grid with the centres of the GLOBAL indices."""
import numpy as np

import tsdf_ref  # tests/tsdf_ref.py

f32 = np.float32
BRICK = (8, 8, 4)
STATE_BYTES_PER_BRICK = 256 * 28


def brick_dims(dims):
    return tuple(-(-int(n) // b) for n, b in zip(dims, BRICK))


def _state_of_seed_bricks(sb):
    """seed bricks (bz, by, bx) bool -> brick_state: 0 none, 1 allocated, 2 seed"""
    bz, by, bx = sb.shape
    pad = np.pad(sb, 1)
    alloc = np.zeros_like(sb)
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                alloc |= pad[dz:dz + bz, dy:dy + by, dx:dx + bx]
    state = alloc.astype(np.uint8)
    state[sb] = 2
    return state


def _seed_bricks(C, shape_bricks):
    """C (nz, ny, nx) of voxels that start at a brick corner -> (bz, by, bx) bool"""
    bz, by, bx = shape_bricks
    seed = np.zeros((bz * BRICK[2], by * BRICK[1], bx * BRICK[0]), bool)
    nz, ny, nx = C.shape
    seed[:nz, :ny, :nx] = C > 0
    return seed.reshape(bz, BRICK[2], by, BRICK[1], bx, BRICK[0]).any(axis=(1, 3, 5))


def allocation(col, dims):
    """The colour sums of the dense field (..., 4) -> brick_state (bz, by, bx)"""
    bx, by, bz = brick_dims(dims)
    return _state_of_seed_bricks(_seed_bricks(np.asarray(col)[..., 3], (bz, by, bx)))


def _voxel_mask(state, shape):
    """brick_state != 0 per voxel of a (nz, ny, nx) array that starts at a brick corner"""
    m = np.repeat(np.repeat(np.repeat(state != 0, BRICK[2], 0), BRICK[1], 1), BRICK[0], 2)
    return m[:shape[0], :shape[1], :shape[2]]


def field_window(cams, cut_maps, images, origin, voxel_size, dims, lo, hi, trunc=0,
                 min_weight=0):
    """Steps 1-8 and F of smvs_tsdf_fuse for the voxels lo <= (i, j, k) < hi of
    a grid of any size -> F, W, col of shape (hi - lo)[::-1]"""
    vs = f32(voxel_size)
    trunc = f32(trunc) if trunc > 0 else f32(3.0) * vs
    min_weight = int(min_weight) if min_weight > 0 else 1
    for a in range(3):
        assert 0 <= lo[a] < hi[a] <= dims[a]
    shape = tuple(int(hi[a] - lo[a]) for a in (2, 1, 0))

    def centres(a):
        return f32(origin[a]) + (np.arange(lo[a], hi[a]).astype(f32) + f32(0.5)) * vs
    cx = np.broadcast_to(centres(0)[None, None, :], shape)
    cy = np.broadcast_to(centres(1)[None, :, None], shape)
    cz = np.broadcast_to(centres(2)[:, None, None], shape)
    S = np.zeros(shape, f32)
    W = np.zeros(shape, np.uint32)
    col = np.zeros(shape + (4,), np.uint32)
    for cam, cut_map, image in zip(cams, cut_maps, images):
        h, w = cut_map.shape
        V = tsdf_ref.camera(cam, w, h)
        D = tsdf_ref.prepared_depth(V, cut_map)
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


def _active_cells(F):
    """the active cells of a field in the order tsdf_ref.surface numbers them
    -> (i, j, k) and their corner values (n, 8)"""
    f = np.stack([tsdf_ref._corner(F, c) for c in range(8)], -1)
    complete = ~np.isnan(f).any(axis=-1)
    with np.errstate(invalid="ignore"):
        n_in = (f < 0).sum(axis=-1)
    active = complete & (n_in != 0) & (n_in != 8)
    kk, jj, ii = np.nonzero(active)
    return (ii, jj, kk), f[active]


def _positions(idx, fa_, origin, voxel_size):
    """the position rule of smvs_tsdf_fuse for cells with the (global) indices idx"""
    vs = f32(voxel_size)
    n = len(idx[0])
    total = [np.zeros(n, f32) for _ in range(3)]
    m = np.zeros(n, np.int32)
    for a, b, axis in tsdf_ref.EDGES:
        Fa, Fb = fa_[:, a], fa_[:, b]
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
    return np.stack([total[r] / m.astype(f32) for r in range(3)], -1).astype(f32)


def sparse_key(i, j, k, dims):
    """(linear brick index) * 256 + the index inside the brick, x fastest"""
    bx, by, _ = brick_dims(dims)
    i, j, k = (np.asarray(x, np.int64) for x in (i, j, k))
    brick = (k // BRICK[2] * by + j // BRICK[1]) * bx + i // BRICK[0]
    return brick * 256 + (k % BRICK[2] * BRICK[1] + j % BRICK[1]) * BRICK[0] + i % BRICK[0]


def reorder(mesh, idx, dims):
    """A mesh in the dense order (tsdf_ref.surface) whose vertex v is the cell
    with the global indices idx[.][v] -> the mesh in the sparse order, cells
    and the permutation (new vertex n is dense vertex perm[n])"""
    nx, ny, _ = (int(x) for x in dims)
    i, j, k = (np.asarray(x, np.int64) for x in idx)
    perm = np.argsort(sparse_key(i, j, k, dims), kind="stable")
    new_id = np.empty(len(perm), np.int64)
    new_id[perm] = np.arange(len(perm))
    out = {key: mesh[key][perm] for key in ("xyz", "normals", "rgb", "confidence")}
    out["cells"] = ((k * ny + j) * nx + i)[perm]
    faces = mesh["faces"].astype(np.int64).reshape(-1, 2, 3)
    if len(faces):
        first, second = faces[:, 0], faces[:, 1]
        v0 = first[:, 0]
        # v2, the cell at the (b, c) offset (0, 0), is the corner both triangles
        # share besides v0: its indices are the grid point's
        shared = (first[:, 1] == second[:, 1]) | (first[:, 1] == second[:, 2])
        v2 = np.where(shared, first[:, 1], first[:, 2])
        p = [i[v2], j[v2], k[v2]]
        same = np.stack([x[v0] == x[v2] for x in (i, j, k)], -1)
        assert np.all(same.sum(axis=1) == 1)
        axis = np.argmax(same, axis=1)
        order = np.argsort(sparse_key(p[0], p[1], p[2], dims) * 3 + axis, kind="stable")
        faces = new_id[faces[order]]
    out["faces"] = faces.reshape(-1, 3).astype(np.uint32)
    return out, perm


def fuse(cams, cut_maps, images, origin, voxel_size, dims, trunc=0, min_weight=0,
         window=None):
    """smvs_tsdf_fuse_sparse on prepared maps -> xyz, normals, rgb, confidence,
    faces, cells, brick_state, stats and, without a window, tsdf and weight.
    window = (lo, hi): voxel indices at brick corners (hi may be dims); the
    caller asserts that no brick outside it is a seed, and its outermost bricks
    inside the grid must hold none either."""
    dims = tuple(int(x) for x in dims)
    bx, by, bz = brick_dims(dims)
    if window is None:
        lo, hi = (0, 0, 0), dims
        F, W, col = tsdf_ref.field(cams, cut_maps, images, origin, voxel_size, dims, trunc,
                                   min_weight)
    else:
        lo, hi = (tuple(int(x) for x in w) for w in window)
        for a in range(3):
            assert lo[a] % BRICK[a] == 0 and (hi[a] % BRICK[a] == 0 or hi[a] == dims[a])
        F, W, col = field_window(cams, cut_maps, images, origin, voxel_size, dims, lo, hi,
                                 trunc, min_weight)
    blo = tuple(lo[a] // BRICK[a] for a in range(3))
    wb = brick_dims(tuple(hi[a] - lo[a] for a in range(3)))
    seeds = _seed_bricks(col[..., 3], wb[::-1])
    if window is not None:
        edge = np.zeros_like(seeds)
        for a, n_all in zip(range(3), (bx, by, bz)):
            sl = [slice(None)] * 3
            if blo[a] > 0:
                sl[2 - a] = 0
                edge[tuple(sl)] = True
            if blo[a] + wb[a] < n_all:
                sl[2 - a] = -1
                edge[tuple(sl)] = True
        assert not (seeds & edge).any(), "a seed in the window's outermost bricks"
    local = _state_of_seed_bricks(seeds)
    state = np.zeros((bz, by, bx), np.uint8)
    state[blo[2]:blo[2] + wb[2], blo[1]:blo[1] + wb[1], blo[0]:blo[0] + wb[0]] = local
    known = _voxel_mask(local, F.shape)
    F = np.where(known, F, f32(np.nan)).astype(f32)
    W = np.where(known, W, 0).astype(np.uint32)
    col = np.where(known[..., None], col, 0).astype(np.uint32)
    dense = tsdf_ref.surface(F, W, col, origin, voxel_size, len(cams))
    idx, fa_ = _active_cells(F)
    idx = tuple(idx[a].astype(np.int64) + lo[a] for a in range(3))
    if window is not None:
        dense["xyz"] = _positions(idx, fa_, origin, voxel_size)
    out, _ = reorder(dense, idx, dims)
    out["brick_state"] = state
    allocated = int((state != 0).sum())
    out["stats"] = {"bricks": bx * by * bz, "seed_bricks": int((state == 2).sum()),
                    "allocated_bricks": allocated,
                    "state_bytes": allocated * STATE_BYTES_PER_BRICK}
    if window is None:
        out["tsdf"] = F
        out["weight"] = W
    return out
