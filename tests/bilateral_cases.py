"""Inputs for the joint bilateral upsample (csrc/bilateral.hip), chosen for the
edges its four forms can get wrong -- no GPU, no smvs_amd.

The filter (depth_optimizer.cc:957-1004): an output pixel (x, y) sums over the
window kx, ky = -k .. k; the tap's guidance pixel is (x + kx, y + ky) clamped
into the image, its depth is dm[(int)(scale_y * ci_y)][(int)(scale_x * ci_x)]
with scale = (float)dm_n / (float)n a float division, a tap without depth
(dv == 0) is skipped, and the weight is gaussian_2d(kx, ky, sigma) times
gaussian(tap - centre, 0.1) per channel, all in float.

  guide()         a u8 guidance image, blocky plus noise, bytes 0 and 255 in it
  low()           a depth map in [2, 3) with scattered zeros and one large hole
  contrast_case() black / white guidance: weight sums that are subnormal, and
                  sums that underflow to zero although taps carry depth
  weight_sums()   float64 restatement of the weight sums, to CLASSIFY pixels
                  (never the expected output: np.exp is not glibc's expf)
  tap_flips()     how many taps move when scale is one ulp off
  CASES           the list the CPU and the GPU tests walk
"""
import collections
import functools

import numpy as np

f32 = np.float32


def guide(w, h, channels, seed):
    """u8 image (h, w) or (h, w, 3): 8 x 8 blocks of random level, every sixth
    of them saturated, plus noise of sigma 6 -- neighbouring bytes differ by
    small and by large amounts.  Contains 0 and 255 (the ends of the table of
    byte pairs)."""
    rng = np.random.default_rng(seed)
    tail = (3,) if channels == 3 else ()
    base = rng.integers(0, 256, size=(h // 8 + 1, w // 8 + 1) + tail).astype(np.float32)
    sat = rng.random(base.shape)
    base[sat < 1.0 / 12.0] = 0.0
    base[sat > 11.0 / 12.0] = 255.0
    img = np.kron(base, np.ones((8, 8) + (1,) * len(tail), np.float32))[:h, :w]
    img = np.clip(img + rng.normal(0, 6, size=img.shape), 0, 255).astype(np.uint8)
    # (an image of a single block need not have reached both ends)
    flat = img.reshape(-1)
    if not (flat == 0).any():
        flat[0] = 0
    if not (flat == 255).any():
        flat[-1] = 255
    return img


def hole_rect(dm_w, dm_h):
    """(x0, y0, x1, y1) of low()'s rectangular hole: the central 60 % of each
    axis; every row when the map has fewer than five (a window then covers the
    whole height, and only a hole of full height leaves an output without
    taps)."""
    hw = max(1, int(np.ceil(0.6 * dm_w)))
    hh = dm_h if dm_h < 5 else int(np.ceil(0.6 * dm_h))
    x0, y0 = (dm_w - hw) // 2, (dm_h - hh) // 2
    return x0, y0, x0 + hw, y0 + hh


def low(dm_w, dm_h, seed, hole=True, zeros=0.2):
    """float32 map in [2, 3), a fraction `zeros` of it scattered holes, and
    (hole=True) the rectangle hole_rect() cleared: wider than the window as
    mapped into the image, so some outputs have no tap at all."""
    rng = np.random.default_rng(seed)
    dm = (2.0 + rng.random((dm_h, dm_w))).astype(np.float32)
    dm[rng.random(dm.shape) < zeros] = 0.0
    if hole:
        x0, y0, x1, y1 = hole_rect(dm_w, dm_h)
        dm[y0:y1, x0:x1] = 0.0
    return dm


def contrast_case():
    """(img u8 45 x 37 x 3, dm 23 x 19).  Left half black, right half white,
    the green channel inverted on every third column of every second row of
    the top 18 rows; the map's left half empty.  Across the edge two channels
    differ by 255 (tap weight ~3.7e-44, subnormal) or three (exactly 0)."""
    img = np.zeros((37, 45, 3), np.uint8)
    img[:, 22:] = 255
    img[0:18:2, ::3, 1] ^= 255
    dm = (2 + np.random.default_rng(1).random((19, 23))).astype(np.float32)
    dm[:, :12] = 0
    return img, dm


def to_float(img):
    """byte_to_float_image: (float)b / 255.0f."""
    return img.astype(np.float32) / f32(255)


def tap_columns(n, dm_n, scale=None):
    """The map index of each of the n guidance columns (or rows), in the
    filter's float arithmetic."""
    if scale is None:
        scale = f32(dm_n) / f32(n)
    fx = f32(scale) * np.arange(n, dtype=np.float32)
    assert fx.dtype == np.float32
    fx = np.minimum(np.maximum(fx, f32(0)), f32(dm_n) - f32(1))
    return fx.astype(np.int32)


def tap_flips(n, dm_n):
    """(down, up): how many of the n columns change their map index when
    (float)dm_n / (float)n is one ulp lower, and when it is one ulp higher."""
    scale = f32(dm_n) / f32(n)
    ref = tap_columns(n, dm_n, scale)
    down = tap_columns(n, dm_n, np.nextafter(scale, f32(-np.inf)))
    up = tap_columns(n, dm_n, np.nextafter(scale, f32(np.inf)))
    return int(np.count_nonzero(down != ref)), int(np.count_nonzero(up != ref))


def weight_sums(dm, ci, sigma, k):
    """(sums float64 (h, w), taps int (h, w)): per output pixel the sum of the
    weights of its depth-bearing taps and their number.  The differences are
    the filter's float32 ones; exponentials, products and sums in float64."""
    dm = np.asarray(dm, np.float32)
    ci = np.asarray(ci, np.float32)
    if ci.ndim == 2:
        ci = ci[:, :, None]
    h, w, _ = ci.shape
    dm_h, dm_w = dm.shape
    col = tap_columns(w, dm_w)
    row = tap_columns(h, dm_h)
    ys, xs = np.arange(h), np.arange(w)
    sums = np.zeros((h, w))
    taps = np.zeros((h, w), np.int64)
    two_s2 = 2.0 * float(f32(sigma)) ** 2
    for ky in range(-k, k + 1):
        cy = np.clip(ys + ky, 0, h - 1)
        for kx in range(-k, k + 1):
            cx = np.clip(xs + kx, 0, w - 1)
            dv = dm[row[cy]][:, col[cx]]
            diff = ci[cy][:, cx] - ci
            assert diff.dtype == np.float32
            d = diff.astype(np.float64)
            wgt = np.exp(-(kx * kx / two_s2 + ky * ky / two_s2)) \
                * np.prod(np.exp(-(d * d) / (2.0 * 0.1 * 0.1)), axis=2)
            has = dv != 0
            sums += np.where(has, wgt, 0.0)
            taps += has
    return sums, taps


def classify(sums, taps):
    """Pixel classes of a case, from weight_sums(): dict of boolean masks.
    The bands leave room for the float32 rounding of products and sums, so a
    pixel near a threshold is in no class."""
    return dict(
        no_taps=taps == 0,
        underflow=(taps > 0) & (sums < 2.0 ** -152),
        subnormal=(sums > 2.0 ** -146) & (sums < 2.0 ** -127),
        normal=sums >= 2.0 ** -120)


Case = collections.namedtuple(
    "Case", "w h dm_w dm_h channels kernel_size sigma name kind")
# kind: how the inputs are made
#   holes     guide() and low() with its rectangular hole
#   scatter   guide() and low() without the rectangle
#   dense     guide() and a map without zeros
#   zero      guide() and an all-zero map
#   contrast  contrast_case(); channels == 1: its green channel


def _case(w, h, dm_w, dm_h, channels, k=5, sigma=5.0, kind="holes"):
    name = "%dx%d_from_%dx%d_c%d_k%d_s%g" % (w, h, dm_w, dm_h, channels, k, sigma)
    if kind != "holes":
        name += "_" + kind
    return Case(w, h, dm_w, dm_h, channels, k, float(sigma), name, kind)


def _build_cases():
    cases = []
    # ragged sizes and ratios where one ulp of scale moves a tap
    for size in [(45, 37, 23, 19), (45, 35, 15, 5), (66, 46, 39, 14), (64, 48, 64, 48),
                 (33, 29, 66, 58)]:
        for c in (3, 1):
            cases.append(_case(*size, c))
    # images narrower than the window; 3 x 3 is the smallest a context takes.
    # A window covers them whole, so no output is without taps: scattered zeros
    # only (7 x 5), none in the single map pixel (3 x 3)
    for c in (3, 1):
        cases.append(_case(7, 5, 3, 2, c, kind="scatter"))
        cases.append(_case(3, 3, 1, 1, c, kind="dense"))
    # wide: four blocks of 256 / two of 1,024, three rows
    for c in (3, 1):
        cases.append(_case(1100, 3, 550, 2, c))
    # other windows (compressed table: 0, 1, 3, 7; generic kernel in a context: 8)
    for k in (0, 1, 3, 7, 8):
        for c in (3, 1):
            cases.append(_case(45, 37, 23, 19, c, k=k))
    # other sigmas.  0.5: a tap five columns and five rows away has the spatial
    # weight exp(-100), below float's normal range, so a pixel that reaches
    # past the rectangular hole only with such taps would have a subnormal sum;
    # the scattered holes alone keep every pixel near a tap with depth
    for c in (3, 1):
        cases.append(_case(45, 37, 23, 19, c, sigma=0.5, kind="scatter"))
        cases.append(_case(45, 37, 23, 19, c, sigma=50.0))
    cases.append(_case(45, 37, 23, 19, 3, kind="contrast"))
    cases.append(_case(45, 37, 23, 19, 1, kind="contrast"))
    for c in (3, 1):
        cases.append(_case(45, 37, 23, 19, c, kind="zero"))
        cases.append(_case(45, 37, 23, 19, c, kind="dense"))
    assert len({c.name for c in cases}) == len(cases)
    return cases


CASES = _build_cases()

# the second trip of the triangle form's persistent grid (one workgroup of 1,024
# lanes per CU; 641 x 417 pixels are more than 256 CUs take in one)
SECOND_TRIP = [_case(641, 417, 321, 209, c) for c in (3, 1)]


def _seed(case):
    return 1000 * case.w + 10 * case.dm_w + case.channels + 100 * case.kernel_size


@functools.lru_cache(maxsize=None)
def _inputs(case):
    if case.kind == "contrast":
        img, dm = contrast_case()
        if case.channels == 1:
            img = np.ascontiguousarray(img[:, :, 1])
    else:
        img = guide(case.w, case.h, case.channels, _seed(case))
        if case.kind == "zero":
            dm = np.zeros((case.dm_h, case.dm_w), np.float32)
        elif case.kind == "dense":
            dm = low(case.dm_w, case.dm_h, _seed(case) + 1, hole=False, zeros=0.0)
        else:
            dm = low(case.dm_w, case.dm_h, _seed(case) + 1, hole=case.kind == "holes")
    img.setflags(write=False)
    dm.setflags(write=False)
    return img, dm


def inputs(case):
    """(img u8, dm float32) of a case: made once, shared, read-only."""
    return _inputs(case)


def has_holes(case):
    """Some outputs of the case have no tap with depth and some have."""
    return case.kind in ("holes", "contrast")


def ulps(got, want):
    """|got - want| in units of want's last place, elementwise (float32, same
    sign or zero)."""
    a = np.asarray(got, np.float32).view(np.int32).astype(np.int64)
    b = np.asarray(want, np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)
