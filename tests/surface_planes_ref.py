"""Numpy restatement of "Node slopes from the SGM plane hypotheses"
(include/smvs_hip.h): the slant plane of a context (the tap rule) and
initialize_node_from_depth with slants, followed by fill_holes and
remove_nodes_without_patch -- Surface::create and fill_patches_from_depth
with a slant plane.  Written from the header's text, array-wise over all nodes
of a grid; it shares no code with csrc/host/surface_math.h.

The other grid operations (expand, subdivide_patches, remove_isolated_patches)
are the reference's and are pinned against the oracle elsewhere; `check_script`
therefore follows a script on the implementation under test and restates every
step that uses the new rule (the create and each fill) from the state before it.
"""
import numpy as np

QNAN = np.uint32(0x7FC00000)


def slant_key(v):
    bits = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    return np.where((bits & np.uint32(0x80000000)) == 0, bits ^ np.uint32(0x80000000), ~bits)


def slant_from_key(k):
    k = np.asarray(k, dtype=np.uint32)
    bits = np.where((k & np.uint32(0x80000000)) != 0, k ^ np.uint32(0x80000000), ~k)
    return bits.astype(np.uint32).view(np.float32)


def tap_plane(lowres, slants, width, height):
    """P (height, width, 2) from L (dm_h, dm_w) and G (dm_h, dm_w, 2)."""
    L = np.asarray(lowres, dtype=np.float32)
    G = np.asarray(slants, dtype=np.float32)
    dm_h, dm_w = L.shape
    f = np.float32
    scale_x = f(dm_w) / f(width)
    scale_y = f(dm_h) / f(height)
    fx = np.clip(scale_x * np.arange(width, dtype=np.float32), f(0), f(dm_w) - f(1))
    fy = np.clip(scale_y * np.arange(height, dtype=np.float32), f(0), f(dm_h) - f(1))
    sx = fx.astype(np.int32)[None, :]
    sy = fy.astype(np.int32)[:, None]
    g = G[sy, sx]                                        # (height, width, 2)
    ok = (L[sy, sx] > 0) & np.isfinite(g[..., 0]) & np.isfinite(g[..., 1])
    out = np.empty((height, width, 2), np.float32)
    out[..., 0] = g[..., 0] * scale_x
    out[..., 1] = g[..., 1] * scale_y
    out.view(np.uint32)[~ok] = QNAN
    return out


def grid_for_scale(width, height, scale):
    ps = 1 << scale
    npx = (width - 2) // ps - 1
    npy = (height - 2) // ps - 1
    return dict(scale=scale, npx=npx, npy=npy, start_x=(width - npx * ps) // 2,
                start_y=(height - npy * ps) // 2)


def clamp_depth(depth):
    d = np.asarray(depth, dtype=np.float32)
    return np.where(d > 0, d, np.float32(0)).astype(np.float32)


def _windows(state, width, height):
    """Pixel coordinates of every node's window: (N, ps, ps) x, y, inside and the
    quadrant index (bit 0: right half, bit 1: lower half)."""
    ps = 1 << state["scale"]
    half = ps // 2
    npx, npy = state["npx"], state["npy"]
    idx = np.tile(np.arange(npx + 1), npy + 1)
    idy = np.repeat(np.arange(npy + 1), npx + 1)
    off = np.arange(ps) - half
    x = (idx * ps + state["start_x"])[:, None, None] + off[None, None, :]
    y = (idy * ps + state["start_y"])[:, None, None] + off[None, :, None]
    x, y = np.broadcast_arrays(x, y)
    inside = (x >= 0) & (x < width) & (y >= 0) & (y < height)
    quad = ((off >= 0).astype(np.int32)[None, None, :]
            + 2 * (off >= 0).astype(np.int32)[None, :, None])
    return x, y, inside, np.broadcast_to(quad, x.shape)


def _node_from_window(median, a, quadrants):
    """lib/surface.cc:703-758 in double, array-wise; a: (N, 4) lowest per quadrant."""
    n = median.shape[0]
    node = np.zeros((n, 4))
    node[:, 0] = median
    a0, a1, a2, a3 = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
    full = quadrants == 4
    dx4 = ((a1 + a3) - (a0 + a2)) / 2.0
    dy4 = ((a2 + a3) - (a0 + a1)) / 2.0
    dxy4 = (a3 - a2) - (a1 - a0)
    c1 = ((a1 == 0) | (a0 == 0)) & (a3 != 0) & (a2 != 0)
    c2 = ((a2 == 0) | (a3 == 0)) & (a1 != 0) & (a0 != 0)
    dxp = np.where(c1, a3 - a2, np.where(c2, a1 - a0, 0.0))
    c3 = ((a0 == 0) | (a2 == 0)) & (a3 != 0) & (a1 != 0)
    c4 = ((a1 == 0) | (a2 == 0)) & (a0 != 0) & (a2 != 0)
    dyp = np.where(c3, a3 - a1, np.where(c4, a2 - a0, 0.0))
    node[:, 1] = np.where(full, dx4, dxp)
    node[:, 2] = np.where(full, dy4, dyp)
    node[:, 3] = np.where(full, dxy4, 0.0)
    return node


def fill_from_depth(state, depth, plane):
    """fill_patches_from_depth on `state` (a dict as host.surface_script returns)
    with D = depth (clamped) and the slant plane P (None: the reference's rule).
    Returns the new state and cs per node (-1 where no node was initialised)."""
    D = clamp_depth(depth)
    height, width = D.shape
    ps = 1 << state["scale"]
    npx, npy = state["npx"], state["npy"]
    nn = (npx + 1) * (npy + 1)
    nodes = np.array(state["nodes"], dtype=np.float64).reshape(nn, 4).copy()
    node_valid = np.array(state["node_valid"], dtype=np.uint8).copy()
    patch_valid = np.array(state["patch_valid"], dtype=np.uint8).copy()
    cs_out = np.full(nn, -1, np.int64)
    if ps >= 2:
        x, y, inside, quad = _windows(state, width, height)
        xc, yc = np.clip(x, 0, width - 1), np.clip(y, 0, height - 1)
        d = D[yc, xc]
        valid = inside & (d > 0)
        n = x.shape[0]
        T = ps * ps
        d2, v2, q2 = d.reshape(n, T), valid.reshape(n, T), quad.reshape(n, T)
        count = v2.sum(axis=1)
        lowest = np.zeros((n, 4))
        quadrants = np.zeros(n, np.int64)
        for q in range(4):
            m = v2 & (q2 == q)
            has = m.any(axis=1)
            low = np.where(m, d2, np.float32(np.inf)).min(axis=1)
            lowest[:, q] = np.where(has, low.astype(np.float64), 0.0)
            quadrants += has
        srt = np.sort(np.where(v2, d2, np.float32(np.inf)), axis=1)
        median = srt[np.arange(n), np.minimum(count // 2, T - 1)].astype(np.float64)
        exists = (quadrants != 0) & (count >= 2)
        node = _node_from_window(np.where(exists, median, 0.0), lowest, quadrants)
        cs = np.zeros(n, np.int64)
        if plane is not None:
            P = np.asarray(plane, dtype=np.float32)
            px, py = P[yc, xc, 0].reshape(n, T), P[yc, xc, 1].reshape(n, T)
            S = v2 & np.isfinite(px) & np.isfinite(py)
            cs = S.sum(axis=1)
            none = np.uint32(0xFFFFFFFF)        # above the key of every finite float
            r = np.minimum(cs // 2, T - 1)
            kx = np.sort(np.where(S, slant_key(px), none), axis=1)[np.arange(n), r]
            ky = np.sort(np.where(S, slant_key(py), none), axis=1)[np.arange(n), r]
            have = cs >= 1
            mx = slant_from_key(np.where(have, kx, np.uint32(0x80000000)))
            my = slant_from_key(np.where(have, ky, np.uint32(0x80000000)))
            node[:, 1] = np.where(have, mx.astype(np.float64) * float(ps), node[:, 1])
            node[:, 2] = np.where(have, my.astype(np.float64) * float(ps), node[:, 2])
            node[:, 3] = np.where(have, 0.0, node[:, 3])
        todo = exists & (node_valid == 0)
        nodes[todo] = node[todo]
        node_valid[todo] = 1
        cs_out[todo] = cs[todo]
    # fill_holes, remove_nodes_without_patch
    nv = node_valid.reshape(npy + 1, npx + 1).astype(bool)
    pv = patch_valid.reshape(npy, npx).astype(bool)
    pv = pv | (nv[:-1, :-1] & nv[:-1, 1:] & nv[1:, :-1] & nv[1:, 1:])
    touched = np.zeros_like(nv)
    touched[:-1, :-1] |= pv
    touched[:-1, 1:] |= pv
    touched[1:, :-1] |= pv
    touched[1:, 1:] |= pv
    nv = nv & touched
    out = dict(state)
    out.update(nodes=nodes, node_valid=nv.reshape(-1).astype(np.uint8),
               patch_valid=pv.reshape(-1).astype(np.uint8))
    return out, cs_out


def create(depth, plane, scale):
    """Surface::create(..., depth, plane)."""
    height, width = np.asarray(depth).shape
    g = grid_for_scale(width, height, scale)
    nn = (g["npx"] + 1) * (g["npy"] + 1)
    g.update(nodes=np.zeros((nn, 4)), node_valid=np.zeros(nn, np.uint8),
             patch_valid=np.zeros(g["npx"] * g["npy"], np.uint8))
    return fill_from_depth(g, depth, plane)


def same_surface(a, b):
    for k in ("scale", "npx", "npy", "start_x", "start_y"):
        assert a[k] == b[k], k
    assert np.array_equal(a["patch_valid"], b["patch_valid"])
    assert np.array_equal(a["node_valid"], b["node_valid"])
    m = np.asarray(a["node_valid"]).astype(bool)
    an = np.asarray(a["nodes"]).reshape(-1, 4)[m]
    bn = np.asarray(b["nodes"]).reshape(-1, 4)[m]
    # (bytes: -0.0 and +0.0 differ)
    assert np.array_equal(an.view(np.uint64), bn.view(np.uint64))


def check_script(run, depth, plane, scale, ops):
    """run(ops) -> the surface of the implementation under test after the script's
    prefix `ops`.  Restates the create and every fill (operation 3) from the state
    before it and compares; returns the cs of the nodes the create initialised."""
    want, cs = create(depth, plane, scale)
    same_surface(run([]), want)
    for k, op in enumerate(ops):
        if op != 3:
            continue
        before = run(list(ops[:k]))
        want_k, _ = fill_from_depth(before, depth, plane)
        same_surface(run(list(ops[:k + 1])), want_k)
    return cs
