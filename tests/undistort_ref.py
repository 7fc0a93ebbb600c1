"""numpy restatement of smvs_undistort_u8 (include/smvs_hip.h): float32
throughout, one array operation per operation of the definition, so that every
intermediate is rounded exactly once.  Shared by the CPU and GPU tests; not
product code."""
import numpy as np

f32 = np.float32

LENS_KEYS = ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2")


def lens_dict(fx, fy, cx, cy, k1=0.0, k2=0.0, p1=0.0, p2=0.0):
    return dict(fx=fx, fy=fy, cx=cx, cy=cy, k1=k1, k2=k2, p1=p1, p2=p2)


def source_positions(lens, width, height, out_focal, out_width, out_height):
    """-> sx, sy (out_height, out_width) float32 and the inside mask."""
    L = {k: f32(lens.get(k, 0.0)) for k in LENS_KEYS}
    inv = f32(1.0 / float(f32(out_focal)))
    x = np.arange(out_width, dtype=np.int64).astype(f32)[None, :]
    y = np.arange(out_height, dtype=np.int64).astype(f32)[:, None]
    half_w = f32(0.5) * f32(out_width)
    half_h = f32(0.5) * f32(out_height)
    u = x + f32(0.5)
    u = u - half_w
    u = u * inv
    v = y + f32(0.5)
    v = v - half_h
    v = v * inv
    u, v = np.broadcast_arrays(u, v)
    uu = u * u
    vv = v * v
    r2 = uu + vv
    uv = u * v
    rad = L["k2"] * r2
    rad = L["k1"] + rad
    rad = r2 * rad
    rad = f32(1.0) + rad
    two_p1 = f32(2.0) * L["p1"]
    two_p2 = f32(2.0) * L["p2"]
    du_a = two_p1 * uv
    du_b = f32(2.0) * uu
    du_b = r2 + du_b
    du_b = L["p2"] * du_b
    du = du_a + du_b
    dv_a = f32(2.0) * vv
    dv_a = r2 + dv_a
    dv_a = L["p1"] * dv_a
    dv_b = two_p2 * uv
    dv = dv_a + dv_b
    sx = u * rad
    sx = sx + du
    sx = L["fx"] * sx
    sx = sx + L["cx"]
    sx = sx - f32(0.5)
    sy = v * rad
    sy = sy + dv
    sy = L["fy"] * sy
    sy = sy + L["cy"]
    sy = sy - f32(0.5)
    for a in (sx, sy):
        assert a.dtype == np.float32
    with np.errstate(invalid="ignore"):
        inside = (sx >= f32(0.0)) & (sx <= f32(width - 1)) & (sy >= f32(0.0)) \
            & (sy <= f32(height - 1))
    return sx, sy, inside


def undistort(image, lens, out_focal, out_size=None):
    """-> (output image, number of blank pixels)."""
    a = np.asarray(image, dtype=np.uint8)
    squeeze = a.ndim == 2
    if squeeze:
        a = a[:, :, None]
    h, w, c = a.shape
    ow, oh = (w, h) if out_size is None else out_size
    sx, sy, inside = source_positions(lens, w, h, out_focal, ow, oh)
    # (positions outside are never sampled: park them on pixel (0, 0))
    sx = np.where(inside, sx, f32(0.0))
    sy = np.where(inside, sy, f32(0.0))
    x0 = sx.astype(np.int64)
    y0 = sy.astype(np.int64)
    x1 = np.minimum(x0 + 1, w - 1)
    y1 = np.minimum(y0 + 1, h - 1)
    w1 = sx - x0.astype(f32)
    w0 = f32(1.0) - w1
    w3 = sy - y0.astype(f32)
    w2 = f32(1.0) - w3
    out = np.zeros((oh, ow, c), np.uint8)
    for ch in range(c):
        v00 = a[y0, x0, ch].astype(f32)
        v10 = a[y0, x1, ch].astype(f32)
        v01 = a[y1, x0, ch].astype(f32)
        v11 = a[y1, x1, ch].astype(f32)
        t0 = v00 * w0
        t0 = t0 * w2
        t1 = v10 * w1
        t1 = t1 * w2
        t2 = v01 * w0
        t2 = t2 * w3
        t3 = v11 * w1
        t3 = t3 * w3
        s = t0 + t1
        s = s + t2
        s = s + t3
        s = s + f32(0.5)
        assert s.dtype == np.float32
        out[:, :, ch] = np.where(inside, s.astype(np.int64), 0).astype(np.uint8)
    blank = int((~inside).sum())
    return (out[:, :, 0] if squeeze else out), blank
