"""Inputs for the scale space (csrc/scale.hip) and a Python mirror of its launch
plan -- no GPU, no smvs_amd.

The file has seven kernels, six compile-time half widths plus a run-time one,
three forms of the x pass, a y pass that exists on its own and fused with the
luminance and the fit, and a byte converter with a tail.  Which of them an
image takes, and on which side of their predicates its workgroups fall, depends
on its width, height and channel count alone; the mirror below restates those
predicates, and the case list is DERIVED from it: the widths and heights that
sit on either side of each of them, at every scale 0 .. 7, grey and RGB.
tests/test_scale_cases_cpu.py checks the constants against the source text and
that every edge is hit; tests/test_gpu_scale_cases.py walks the list.

  half_width(scale), x_form(scale), has_fused(scale)   which kernels a scale takes
  x_blocks, x_interior, lds_x_first                    the x pass of a row
  fused_tiles, fused_inner                             the fused y pass
  y_row_blocks, grad_blocks, converter                 the rest
  sizes(scale, c)                                      [(w, h, group)], derived
  images(w, h, c, group)                               {content name: u8 image}
"""
import functools

import numpy as np

import scale_ref  # tests/scale_ref.py

# csrc/scale.hip's constants (test_scale_cases_cpu.py reads them from the source)
BLOCK = 256               # elements of a row per workgroup (x pass), threads
BLUR_X_ROWS = 4           # image rows per workgroup, per-thread-loads x pass
BLUR_ROWS = 4             # output rows per thread of blur_y_kernel
BLUR_X_LDS_FROM = 12      # half width from which the x pass stages its row in LDS
FUSE_ROWS = 9
FUSE_COLS = 254
GRAD_ROWS = 8
COMPILED_HALF_WIDTHS = (1, 2, 4, 7, 12, 23)     # launch_blur's switch
FUSED_HALF_WIDTHS = (1, 2, 4, 7, 12)            # launch_blur_gradients' switch
MAX_TAPS = 64             # BlurTaps::k
ASYNC_FROM = 1 << 20      # bytes from which upload_image_async defers the conversion

SCALES = tuple(range(8))
CHANNELS = (3, 1)

half_width = scale_ref.half_width


def x_form(scale):
    """'rows': four rows per thread where interior, compile-time width;
    'lds': the row segment staged in LDS; 'runtime': blur_x_kernel<C, 0, 4>."""
    ks = half_width(scale)
    if ks not in COMPILED_HALF_WIDTHS:
        return "runtime"
    return "lds" if ks >= BLUR_X_LDS_FROM else "rows"


def has_fused(scale):
    return half_width(scale) in FUSED_HALF_WIDTHS


def refused(scale):
    """smvs_ctx_set_scale: "blur kernel too wide"."""
    return half_width(scale) + 1 > MAX_TAPS


def x_blocks(w, c):
    return (w * c + BLOCK - 1) // BLOCK


def x_interior(w, c, ks, block):
    """blur_x_kernel's `interior` of workgroup `block` of a row."""
    e0 = block * BLOCK
    return e0 // c - ks >= 0 and (e0 + BLOCK - 1) // c + ks <= w - 1


def x_interior_blocks(w, c, ks):
    return [b for b in range(x_blocks(w, c)) if x_interior(w, c, ks, b)]


def lds_x_first(c, block):
    """First pixel of an LDS-form workgroup; its first element's channel."""
    e0 = block * BLOCK
    return e0 // c, e0 % c


def fused_tiles(w, h):
    return (w + FUSE_COLS - 1) // FUSE_COLS, (h + FUSE_ROWS - 1) // FUSE_ROWS


def fused_inner(h, ks, tile_y):
    """blur_y_gradients_kernel's `inner` of tile row `tile_y`."""
    y0 = tile_y * FUSE_ROWS
    return y0 - 1 - ks >= 0 and y0 + FUSE_ROWS + ks <= h - 1


def fused_inner_tiles(h, ks):
    return [t for t in range(fused_tiles(1, h)[1]) if fused_inner(h, ks, t)]


def y_row_blocks(h):
    return (h + BLUR_ROWS - 1) // BLUR_ROWS


def y_block_clamps(h, ks, block):
    """(low, high): blur_y_kernel's row block reads rows clamped at the top,
    at the bottom."""
    y0 = block * BLUR_ROWS
    return y0 - ks < 0, y0 + ks + BLUR_ROWS - 1 > h - 1


def grad_blocks(w, h):
    return (w + BLOCK - 1) // BLOCK, (h + GRAD_ROWS - 1) // GRAD_ROWS


def converter(n):
    """(chunks of 16 bytes, tail bytes) of byte_to_float16_kernel."""
    return n // 16, n % 16


def first_interior_width(c, ks):
    """w1: the smallest width at which workgroup 1 of the x pass is interior
    (workgroup 0 never is: its first pixel has no left neighbour)."""
    w = 3
    while not (x_blocks(w, c) > 1 and x_interior(w, c, ks, 1)):
        w += 1
    return w


def first_inner_height(ks):
    """h1: the smallest height with an inner tile row of the fused pass."""
    h = 3
    while not fused_inner_tiles(h, ks):
        h += 1
    return h


def lds_widths(c):
    """Widths whose rows are 255, 256, 257 and 513 elements -- one workgroup not
    quite full, full, a second of one element, a third that starts past pixel 0
    -- or, where the channel count does not divide the figure, the next width
    up (RGB: 85, 86, 171 for 255, 258, 513 elements; workgroup 2 then starts at
    element 512 = pixel 170, channel 2: in the middle of a pixel)."""
    return sorted({(e + c - 1) // c for e in (255, 256, 257, 513)})


SEAM_WIDTHS = (254, 255, 256, 257, 258)     # fused tile 1 begins at pixel 254, block 1 at 256
SEAM_HEIGHTS = (9, 10, 11)                  # fused tile row 1 begins at row 9
SMALL = ((3, 3), (3, 4), (4, 3), (5, 4))    # (w, h): fewer than 16 bytes when grey, but 5 x 4


@functools.lru_cache(maxsize=None)
def sizes(scale, c):
    """[(w, h, group)] of a scale and channel count.  group 'edge': random bytes
    only; 'seam' and 'small': every content of images()."""
    ks = half_width(scale)
    out = []

    def add(w, h, group):
        if (w, h) not in [(a, b) for a, b, _ in out]:
            out.append((w, h, group))

    for w, h in SMALL:
        add(w, h, "small")
    # narrower and shorter than the half width: both clamps act in one tap loop
    # (3 x 3 is the smallest image a context takes; at half widths 1 and 2
    # nothing is narrower, and at 2 the middle column of 3 x 3 clamps both ways)
    if ks > 3:
        add(ks - 1, ks - 1, "small")
    for w in SEAM_WIDTHS:
        add(w, 11, "seam")
    for h in SEAM_HEIGHTS:
        add(5, h, "seam")
    # the x pass; six rows: a second row group of two rows
    if x_form(scale) == "lds":
        for w in lds_widths(c):
            add(w, 5, "edge")
    else:
        w1 = first_interior_width(c, ks)
        add(w1 - 1, 6, "edge")
        add(w1, 6, "edge")
    add(BLOCK // c + 1, 6, "edge")          # two workgroups per row
    # the y pass
    if has_fused(scale):
        h1 = first_inner_height(ks)
        add(5, h1 - 1, "edge")
        add(5, h1, "edge")
    else:
        for h in (8, 9, 10, 2 * ks + 4, 2 * ks + 5):
            add(5, h, "edge")
    return tuple(out)


CONTENTS = ("random", "white", "grey128", "zero", "checker", "impulse_corner", "impulse_seam",
            "ramp")


def _seed(w, h, c):
    return 100000 * w + 10 * h + c


@functools.lru_cache(maxsize=None)
def _images(w, h, c, group):
    shape = (h, w, 3) if c == 3 else (h, w)
    rng = np.random.default_rng(_seed(w, h, c))
    out = {"random": rng.integers(0, 256, size=shape).astype(np.uint8)}
    if group != "edge":
        out["white"] = np.full(shape, 255, np.uint8)
        out["grey128"] = np.full(shape, 128, np.uint8)
        out["zero"] = np.zeros(shape, np.uint8)
        ys, xs = np.mgrid[0:h, 0:w]
        checker = (((xs + ys) & 1) * 255).astype(np.uint8)
        out["checker"] = np.repeat(checker[:, :, None], 3, axis=2) if c == 3 else checker
        corner = np.zeros(shape, np.uint8)
        corner[0, 0] = 255
        out["impulse_corner"] = corner
        # the last pixel of fused tile (0, 0) -- pixel 253 of row 8 -- or the
        # image's far corner where it is smaller
        seam = np.zeros(shape, np.uint8)
        seam[min(FUSE_ROWS - 1, h - 1), min(FUSE_COLS - 1, w - 1)] = 255
        out["impulse_seam"] = seam
        ramp = np.arange(w, dtype=np.int64)[None, :].repeat(h, axis=0)
        if c == 3:
            out["ramp"] = np.stack([ramp % 256, (3 * ramp + 85) % 256, 255 - ramp % 256],
                                   axis=2).astype(np.uint8)
        else:
            out["ramp"] = (ramp % 256).astype(np.uint8)
    for img in out.values():
        img.setflags(write=False)
    return out


def images(w, h, c, group):
    """{content: u8 image (h, w) or (h, w, 3)}: made once, shared, read-only."""
    return _images(w, h, c, group)


def stacked(w, h, c, group):
    """(names, (n, h, w[, 3]) u8) of images()."""
    imgs = images(w, h, c, group)
    names = tuple(imgs)
    return names, np.stack([imgs[k] for k in names])


def first_difference(got, want):
    """None, or (number of differing floats, index of the first, both values)
    of two float32 arrays compared by bit pattern."""
    bad = np.argwhere(scale_ref.bits(got) != scale_ref.bits(want))
    if len(bad) == 0:
        return None
    at = tuple(int(i) for i in bad[0])
    return len(bad), at, got[at], want[at]
