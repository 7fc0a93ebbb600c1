"""The definition of the persistent fusion volume (the comment of
smvs_tsdf_volume_create in include/smvs_hip.h) restated in numpy float32 with
explicit state, on top of tests/tsdf_ref.py: the surface is tsdf_ref.surface,
the field loop is a copy of tsdf_ref.field's that starts from the stored sums
and keeps S instead of dividing.

A state is a dict: the grid (origin, voxel_size, dims, trunc), S (nz, ny, nx)
float32, W uint32, rgbc (nz, ny, nx, 4) uint32 (R, G, B, C) and n_views.
integrate returns a new state and leaves its argument alone.  As in
tsdf_ref.py the inputs are the PREPARED maps: the cut maps of the batch (the
cut acts within a batch), or the depth maps where nothing is cut."""
import numpy as np

import tsdf_ref  # tests/tsdf_ref.py

f32 = np.float32


def create(origin, voxel_size, dims, trunc=0):
    nx, ny, nz = (int(x) for x in dims)
    shape = (nz, ny, nx)
    return {"origin": tuple(origin), "voxel_size": voxel_size, "dims": (nx, ny, nz),
            "trunc": trunc, "S": np.zeros(shape, f32), "W": np.zeros(shape, np.uint32),
            "rgbc": np.zeros(shape + (4,), np.uint32), "n_views": 0}


def integrate(state, cams, cut_maps, images, batch_local=False):
    """Field, steps 1-8 for the views of one batch in list order, from the
    stored sums.  batch_local is the WRONG operation order, for the tests that
    show the right one matters: the batch's terms summed on their own from
    0.0f and then added to the stored S (S0 + (a + b) instead of (S0 + a) + b)."""
    nx, ny, nz = state["dims"]
    origin = state["origin"]
    vs = f32(state["voxel_size"])
    trunc = f32(state["trunc"]) if state["trunc"] > 0 else f32(3.0) * vs
    shape = (nz, ny, nx)
    cx = np.broadcast_to(tsdf_ref._centres(origin, vs, nx, 0)[None, None, :], shape)
    cy = np.broadcast_to(tsdf_ref._centres(origin, vs, ny, 1)[None, :, None], shape)
    cz = np.broadcast_to(tsdf_ref._centres(origin, vs, nz, 2)[:, None, None], shape)
    S = np.zeros(shape, f32) if batch_local else state["S"].copy()
    W = state["W"].copy()
    col = state["rgbc"].copy()
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
    if batch_local:
        S = (state["S"] + S).astype(f32)
    out = dict(state)
    out.update(S=S.astype(f32), W=W, rgbc=col, n_views=state["n_views"] + len(cams))
    return out


def field(state, min_weight=0):
    """F = S / (float)W where W >= min_weight, else NaN"""
    min_weight = int(min_weight) if min_weight > 0 else 1
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(state["W"] >= min_weight, state["S"] / state["W"].astype(f32),
                        f32(np.nan)).astype(f32)


def extract(state, min_weight=0):
    """smvs_tsdf_volume_extract -> the mesh dict plus tsdf and weight"""
    F = field(state, min_weight)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = tsdf_ref.surface(F, state["W"], state["rgbc"], state["origin"],
                               state["voxel_size"], state["n_views"])
    out["tsdf"] = F
    out["weight"] = state["W"]
    return out


def fuse_batches(batches, origin, voxel_size, dims, trunc=0, batch_local=False):
    """create, then integrate per (cams, cut_maps, images) batch -> the state"""
    state = create(origin, voxel_size, dims, trunc)
    for cams, cut_maps, images in batches:
        state = integrate(state, cams, cut_maps, images, batch_local=batch_local)
    return state
