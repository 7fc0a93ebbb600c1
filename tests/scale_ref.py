"""StereoView::set_scale (lib/stereo_view.cc:24-46, 97-188) restated in float32
numpy, operation by operation -- no GPU, no smvs_amd, no oracle.

The CPU oracle's blur is marked [MVE-unverified] and was the only statement of
these planes; this is a second, independent reading of the same few lines,
pinned against it to the bit by tests/test_scale_cases_cpu.py:

  bytes       (float)b / 255.0f
  sigma       (float)(0.12 * 2^scale + 0.2), half width ceil(sigma * 2.884f)
  taps        expf(-((float)i * (float)i) / (2.0f * sigma * sigma)), i = 0 .. ks,
              from libm's expf through ctypes: np.exp on float32 is an ulp away
              from glibc at some arguments, and seven of the eight scales show it
  blur        x then y; per element av = av + v * k over the taps -ks .. ks in
              ascending order with the index clamped into the image, the weight
              total aw = aw + k summed in float in the same order, result av / aw
  luminance   (r * 0.21f + g * 0.72f) + b * 0.07f; a grey image is its own
  fit         the 3 x 3 window as nine doubles, x offset a outer and y offset b
              inner; each row of the 6 x 9 matrix summed from 0.0 in column
              order; gradient ((float)r3, (float)r4), Hessian ((float)(2 r0),
              (float)r2, (float)(2 r1)); the image's rim stays zero

planes() also takes one keyword per way a kernel could be wrong while staying
close: a result equal to a variant's names the kind of error.

  descending    the taps from +ks down to -ks
  contracted    multiply-add without the product's rounding (blur and luminance):
                the product is exact in double, the sum is rounded to double
                and then to float -- an FMA but for rare double roundings
  wsum_double   the weight total summed in double, rounded to float once
  y_first       the y pass before the x pass
  reflect       borders mirrored (-1 -> 1) instead of clamped
  swap_window   the window walked with b outer and a inner (the matrix columns
                permuted with it): the same terms summed in another order
"""
import ctypes
import ctypes.util

import numpy as np

f32 = np.float32
VARIANTS = ("descending", "contracted", "wsum_double", "y_first", "reflect", "swap_window")

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.expf.restype = ctypes.c_float
_libm.expf.argtypes = [ctypes.c_float]


def sigma_of(scale):
    """(float)(0.12 * pow(2.0, scale) + 0.2)."""
    return f32(0.12 * 2.0 ** scale + 0.2)


def half_width(scale):
    """ceil(sigma * 2.884f), the product in float."""
    return int(np.ceil(sigma_of(scale) * f32(2.884)))


def taps(scale):
    """The weights k[0 .. ks] as float32."""
    sigma = sigma_of(scale)
    ks = half_width(scale)
    den = f32(2.0) * sigma * sigma
    assert den.dtype == np.float32
    k = np.zeros(ks + 1, np.float32)
    for i in range(ks + 1):
        arg = -(f32(i) * f32(i)) / den
        assert arg.dtype == np.float32
        k[i] = _libm.expf(float(arg))
    return k


def weight_total(k, wsum_double=False, descending=False):
    """aw = aw + k[|i|] over the taps, in float (Accum<float>)."""
    ks = len(k) - 1
    order = range(ks, -ks - 1, -1) if descending else range(-ks, ks + 1)
    aw = np.float64(0.0) if wsum_double else f32(0.0)
    for i in order:
        aw = aw + (np.float64(k[abs(i)]) if wsum_double else k[abs(i)])
    return f32(aw)


def _madd(av, v, k, contracted):
    if contracted:
        return (av.astype(np.float64) + v.astype(np.float64) * np.float64(k)).astype(np.float32)
    return av + v * k


def _border(idx, n, reflect):
    if not reflect:
        return np.clip(idx, 0, n - 1)
    if n == 1:
        return np.zeros_like(idx)
    period = 2 * (n - 1)
    idx = np.mod(idx, period)
    return np.where(idx > n - 1, period - idx, idx)


def _blur_axis(img, axis, k, aw, descending, contracted, reflect):
    """One separable pass of a (batch, h, w, c) float32 array along `axis`."""
    ks = len(k) - 1
    n = img.shape[axis]
    at = np.arange(n)
    av = np.zeros_like(img)
    order = range(ks, -ks - 1, -1) if descending else range(-ks, ks + 1)
    for i in order:
        v = np.take(img, _border(at + i, n, reflect), axis=axis)
        av = _madd(av, v, k[abs(i)], contracted)
        assert av.dtype == np.float32
    return av / aw


def blurred(img_f32, scale, descending=False, contracted=False, wsum_double=False,
            y_first=False, reflect=False):
    """mve::image::blur_gaussian<float> of a (batch, h, w, c) float32 array."""
    sigma = sigma_of(scale)
    if abs(sigma) < f32(0.1):
        return img_f32.copy()
    k = taps(scale)
    aw = weight_total(k, wsum_double, descending)
    for axis in ((1, 2) if y_first else (2, 1)):
        img_f32 = _blur_axis(img_f32, axis, k, aw, descending, contracted, reflect)
    return img_f32


def luminance(img_f32, contracted=False):
    """DESATURATE_LUMINANCE of (batch, h, w, c): (batch, h, w) float32."""
    if img_f32.shape[3] < 3:
        return img_f32[..., 0]
    r, g, b = img_f32[..., 0], img_f32[..., 1], img_f32[..., 2]
    lum = r * f32(0.21)
    lum = _madd(lum, g, f32(0.72), contracted)
    lum = _madd(lum, b, f32(0.07), contracted)
    assert lum.dtype == np.float32
    return lum


def fit_matrix():
    """Rows xx, yy, xy, x, y, 1 over the columns (a, b), a outer and b inner."""
    m = np.zeros((6, 9))
    col = 0
    for a in (-1, 0, 1):
        for b in (-1, 0, 1):
            m[0, col] = -1.0 / 3.0 if a == 0 else 1.0 / 6.0
            m[1, col] = -1.0 / 3.0 if b == 0 else 1.0 / 6.0
            m[2, col] = 0.0 if a * b == 0 else (1.0 / 4.0 if a * b > 0 else -1.0 / 4.0)
            m[3, col] = 0.0 if a == 0 else (1.0 / 6.0 if a > 0 else -1.0 / 6.0)
            m[4, col] = 0.0 if b == 0 else (1.0 / 6.0 if b > 0 else -1.0 / 6.0)
            m[5, col] = 5.0 / 9.0 if (a == 0 and b == 0) else (
                2.0 / 9.0 if (a == 0 or b == 0) else -1.0 / 9.0)
            col += 1
    return m


def gradients_and_hessian(lum, swap_window=False):
    """compute_gradients_and_hessian of (batch, h, w) float32: ((batch, h, w, 2),
    (batch, h, w, 3)) float32."""
    n, h, w = lum.shape
    grad = np.zeros((n, h, w, 2), np.float32)
    hess = np.zeros((n, h, w, 3), np.float32)
    m = fit_matrix()
    window = [(a, b) for a in (-1, 0, 1) for b in (-1, 0, 1)]
    walk = list(range(9))
    if swap_window:
        walk = [window.index((a, b)) for b in (-1, 0, 1) for a in (-1, 0, 1)]
    wide = lum.astype(np.float64)
    r = [np.zeros((n, h - 2, w - 2)) for _ in range(5)]
    for i in walk:
        a, b = window[i]
        v = wide[:, 1 + b:h - 1 + b, 1 + a:w - 1 + a]
        for row in range(5):
            r[row] = r[row] + m[row, i] * v
    inner = (slice(None), slice(1, h - 1), slice(1, w - 1))
    grad[inner + (0,)] = r[3].astype(np.float32)
    grad[inner + (1,)] = r[4].astype(np.float32)
    hess[inner + (0,)] = (2.0 * r[0]).astype(np.float32)
    hess[inner + (1,)] = r[2].astype(np.float32)
    hess[inner + (2,)] = (2.0 * r[1]).astype(np.float32)
    return grad, hess


def planes_batch(imgs_u8, scale, descending=False, contracted=False, wsum_double=False,
                 y_first=False, reflect=False, swap_window=False):
    """planes() of several images of one size at once: (batch, h, w[, c]) u8."""
    imgs = np.asarray(imgs_u8)
    assert imgs.dtype == np.uint8
    if imgs.ndim == 3:
        imgs = imgs[..., None]
    img = imgs.astype(np.float32) / f32(255.0)
    assert img.dtype == np.float32
    blur = blurred(img, scale, descending, contracted, wsum_double, y_first, reflect)
    return gradients_and_hessian(luminance(blur, contracted), swap_window)


def planes(img_u8, scale, **variant):
    """(gradient (h, w, 2), Hessian (h, w, 3)) float32 of a (h, w) or (h, w, c)
    u8 image at `scale`; variant: one of VARIANTS = True."""
    grad, hess = planes_batch(np.asarray(img_u8)[None], scale, **variant)
    return grad[0], hess[0]


def bits(a):
    """The float32 array's bit patterns: -0 and +0 differ, a NaN equals itself."""
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.uint32)
