"""Inputs on which the last two tests of the visibility kernel
(csrc/topo_visibility.hip: warp anisotropy, ncc_for_patch) actually decide --
plain numpy, no GPU; walked by test_visibility_cases_cpu.py (the oracle alone:
every case is non-vacuous and well-conditioned) and by
test_gpu_visibility_decisions.py (the device against the oracle's masks).

Geometry is synth's: ring cameras around a SphereScene, a node grid from the
analytic depth, every patch and node valid.  The IMAGES are the case's own u8
arrays (uploaded as bytes, handed to the oracle as u8 / 255 in float32); on
synth's renderings of the true scene the NCC is far above zero everywhere and
decides nothing.  All views of a case have the main view's size.

  noise      independent uniform u8 noise per view, RGB: the sign of the NCC is
             a coin flip per pair, so one wrong tap, weight, channel, mean or
             reduction moves many mask bits; one case per scale 0 .. 6
  channels   the same with 1- and 3-channel views mixed (the channel clamps)
  bands      noise, with a block of patches on which every view is one constant
             (ncc = 1 by the norm test) and a block under which the neighbours
             are zero bytes (norm1 == 0, dot == 0: 0 / 0 = NaN, not < 0)
  border     image sizes and a shorter neighbour focal length at which the rim
             patches survive the border test: the sample templates other than
             the interior one (scales 0 and 1 only)
  outside    images so small that the 3 % border is under two pixels: the
             +-2 pixel rim samples leave [1, w - 2]
  anisotropy node derivatives perturbed until the warp's ratio of squared
             singular values passes 8
"""
import collections
import functools

import numpy as np

Case = collections.namedtuple(
    "Case", "name family w h n_subs scale sets channels bands sub_flen slope_noise seed")


def _case(name, family, w, h, n_subs, scale, sets=1, channels=None, bands=False,
          sub_flen=1.2, slope_noise=0.0, seed=None):
    if channels is None:
        channels = (3,) * (n_subs + 1)
    if seed is None:
        seed = 1000 * scale + w
    return Case(name, family, w, h, n_subs, scale, sets, tuple(channels), bands,
                sub_flen, slope_noise, seed)


# (size per scale: the smallest that still gives the pair counts the CPU test
# asks for; scales 5 and 6 have few patches, so they hold several image sets on
# one geometry -- as many as the sensitivity bound of the CPU test needs)
NOISE = [
    _case("noise_s0", "noise", 96, 80, 4, 0),
    _case("noise_s1", "noise", 161, 128, 4, 1),
    _case("noise_s2", "noise", 320, 256, 4, 2),
    _case("noise_s3", "noise", 384, 256, 4, 3),
    _case("noise_s4", "noise", 512, 384, 4, 4),
    _case("noise_s5", "noise", 576, 416, 4, 5, sets=2),
    _case("noise_s6", "noise", 960, 704, 8, 6, sets=2),
]

CHANNELS = [
    _case("grey_s2", "channels", 320, 256, 4, 2, channels=(1, 1, 1, 1, 1)),
    _case("rgb_main_grey_subs_s2", "channels", 320, 256, 4, 2, channels=(3, 1, 1, 1, 1)),
    _case("grey_main_rgb_subs_s2", "channels", 320, 256, 4, 2, channels=(1, 3, 3, 3, 3)),
    _case("alternating_s2", "channels", 320, 256, 4, 2, channels=(3, 1, 3, 1, 3)),
]

BANDS = [
    _case("bands_s2", "bands", 320, 256, 4, 2, bands=True),
    _case("bands_s4", "bands", 512, 384, 4, 4, bands=True),
]

BORDER = [
    _case("border_s0_97x80", "border", 97, 80, 4, 0, sub_flen=0.9),
    _case("border_s1_161x128", "border", 161, 128, 4, 1, sub_flen=0.9),
    _case("border_s1_160x129", "border", 160, 129, 4, 1, sub_flen=0.9),
]

OUTSIDE = [
    _case("outside_s0_64x48", "outside", 64, 48, 4, 0),
    _case("outside_s1_64x48", "outside", 64, 48, 4, 1),
    _case("outside_s2_64x48", "outside", 64, 48, 4, 2),
    _case("outside_s1_48x40", "outside", 48, 40, 4, 1),
]

ANISOTROPY = [
    _case("anisotropy_s2", "anisotropy", 320, 256, 4, 2, slope_noise=0.3),
    _case("anisotropy_s4", "anisotropy", 512, 384, 4, 4, slope_noise=1.0, seed=4006),
    # (patches of 64 pixels on the sphere's rim are slanted enough as they are)
    _case("anisotropy_s6", "anisotropy", 960, 704, 8, 6, sets=2, seed=6961),
]

CASES = NOISE + CHANNELS + BANDS + BORDER + OUTSIDE + ANISOTROPY
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# The sample templates (csrc/host/topo_math.h, ncc_flags: 1 corners, 2 top,
# 4 bottom, 8 left, 16 right; 31 is an interior patch) that occur in each border
# case.  Surface::Surface centres the grid, so at scale 0 a patch can sit one
# or two pixels from the image's edge, at scale 1 two or three: width and
# height parity decide which.
BORDER_TEMPLATES = {
    "border_s0_97x80": (10, 11, 12, 13, 14, 15, 18, 19, 20, 21, 22, 23, 26, 27, 28, 29, 31),
    "border_s1_161x128": (10, 13, 15, 18, 21, 23, 26, 29, 31),
    "border_s1_160x129": (10, 12, 14, 19, 21, 23, 27, 29, 31),
}


def ids(cases):
    return [c.name for c in cases]


def template_flags(surf):
    """ncc_for_patch's five border predicates (depth_optimizer.cc:812-857) per
    patch, as one number: 1 corner samples, 2 / 4 / 8 / 16 the two extra rows
    above / below, columns left / right of the patch."""
    ps = 1 << surf["scale"]
    w, h = surf["width"], surf["height"]
    p = np.arange(surf["npx"] * surf["npy"])
    min_x = surf["start_x"] + (p % surf["npx"]) * ps
    min_y = surf["start_y"] + (p // surf["npx"]) * ps
    max_x, max_y = min_x + ps, min_y + ps
    f = ((min_x > 1) & (max_x < w - 2) & (min_y > 1) & (max_y < h - 2)) * 1
    f = f | (min_y > 2) * 2 | (max_y < h - 3) * 4 | (min_x > 2) * 8 | (max_x < w - 3) * 16
    return f.astype(np.int32)


@functools.lru_cache(maxsize=None)
def geometry(case):
    """Cameras, reprojections and the all-valid surface of a case (shared by
    its image sets; treat as read-only)."""
    from smvs_amd import synth
    main, _ = synth.ring_cameras(case.w, case.h, case.n_subs, flen=1.2)
    _, subs = synth.ring_cameras(case.w, case.h, case.n_subs, flen=case.sub_flen)
    scene = synth.SphereScene(seed=2000, px_size=3.0 / (main.flen * max(case.w, case.h)))
    surf = synth.surface_from_depth(scene, main, subs, case.scale, noise=0.01)
    if case.slope_noise > 0:
        rng = np.random.default_rng(case.seed + 77)
        nodes = surf["nodes"].copy()
        nodes[:, 1:4] += case.slope_noise * rng.standard_normal((nodes.shape[0], 3))
        surf["nodes"] = nodes
    surf["patch_valid"] = np.ones_like(surf["patch_valid"])
    surf["node_valid"] = np.ones_like(surf["node_valid"])
    surf["patch_vis"] = np.zeros_like(surf["patch_vis"])
    Ms, ts = zip(*[synth.reprojection(main, s) for s in subs])
    K = main.K(np.float32)
    zero2 = np.zeros((case.h, case.w, 2), np.float32)
    zero3 = np.zeros((case.h, case.w, 3), np.float32)
    # (what ViewContext.set_views wants: the cameras; the planes are replaced
    # by the device's own scale space of the uploaded images)
    views = dict(flen=float(K[0, 0]), inv_flen=float(main.Kinv(np.float32)[0, 0]),
                 grad=zero2, subs=[(zero2, zero3)] * case.n_subs, M=np.array(Ms),
                 t=np.array(ts), shading=None, shading_grad=None)
    return dict(main=main, subs=subs, surf=surf, views=views, M=np.array(Ms), t=np.array(ts))


def _block_patches(case, x_lo, x_hi):
    """The patches whose pixels lie in columns [x_lo * w, x_hi * w) and rows
    [0.1 h, 0.9 h): (first column, first row, columns, rows) of the grid."""
    surf = geometry(case)["surf"]
    ps = 1 << case.scale
    cols = [c for c in range(surf["npx"]) if surf["start_x"] + c * ps >= x_lo * case.w
            and surf["start_x"] + (c + 1) * ps <= x_hi * case.w]
    rows = [r for r in range(surf["npy"]) if surf["start_y"] + r * ps >= 0.1 * case.h
            and surf["start_y"] + (r + 1) * ps <= 0.9 * case.h]
    return cols[0], rows[0], len(cols), len(rows)


def band_blocks(case):
    """(flat block, zero block) of a `bands` case: rectangles of the patch grid
    on the background plane left and right of the sphere, where the surface is
    smooth and the footprint of a block in a neighbour is known to a fraction
    of a pixel.  The sphere's silhouette spans the columns 0.2 w .. 0.8 w of
    the main view and its rim moves 0.04 w further than the plane between the
    views: the blocks keep 0.07 w away, so that no patch of the sphere lands
    on a block's footprint."""
    return _block_patches(case, 0.05, 0.13), _block_patches(case, 0.87, 0.95)


def block_pixels(case, block):
    """(x0, y0, x1, y1): the main view's pixels ncc_for_patch reads for the
    patches of a block -- theirs and the two-pixel rim of samples around."""
    surf = geometry(case)["surf"]
    ps = 1 << case.scale
    c0, r0, nc, nr = block
    x0, y0 = surf["start_x"] + c0 * ps, surf["start_y"] + r0 * ps
    return x0 - 2, y0 - 2, x0 + nc * ps + 3, y0 + nr * ps + 3


def block_footprint(case, block, j):
    """Boolean (h, w): the pixels of neighbour j that the bilinear taps of a
    block's samples can touch, and one pixel around them.  The depth of a
    sample is taken from the node depths, bilinear, clamped to the block (a rim
    sample has the depth of the patch's edge pixel): on the background plane
    that is within a fraction of a pixel of the bicubic surface's warp."""
    g = geometry(case)
    surf = g["surf"]
    ps = 1 << case.scale
    c0, r0, nc, nr = block
    f = surf["nodes"][:, 0].reshape(surf["npy"] + 1, surf["npx"] + 1)
    x0, y0, x1, y1 = block_pixels(case, block)
    X, Y = np.meshgrid(np.arange(x0, x1, dtype=float), np.arange(y0, y1, dtype=float))
    u = np.clip((X + 0.5 - surf["start_x"]) / ps, c0, c0 + nc - 1e-9)
    v = np.clip((Y + 0.5 - surf["start_y"]) / ps, r0, r0 + nr - 1e-9)
    iu, iv = u.astype(int), v.astype(int)
    a, b = u - iu, v - iv
    d = (f[iv, iu] * (1 - a) * (1 - b) + f[iv, iu + 1] * a * (1 - b)
         + f[iv + 1, iu] * (1 - a) * b + f[iv + 1, iu + 1] * a * b)
    M, t = g["M"][j].reshape(3, 3), g["t"][j]
    px, py = X + 0.5, Y + 0.5
    qa = d * (M[0, 0] * px + M[0, 1] * py + M[0, 2]) + t[0]
    qb = d * (M[1, 0] * px + M[1, 1] * py + M[1, 2]) + t[1]
    qc = d * (M[2, 0] * px + M[2, 1] * py + M[2, 2]) + t[2]
    fx = np.floor(qa / qc - 0.5).astype(int)
    fy = np.floor(qb / qc - 0.5).astype(int)
    out = np.zeros((case.h, case.w), bool)
    for dy in range(-1, 3):
        for dx in range(-1, 3):
            yy, xx = fy + dy, fx + dx
            ok = (yy >= 0) & (yy < case.h) & (xx >= 0) & (xx < case.w)
            out[yy[ok], xx[ok]] = True
    return out


FLAT_BYTE = 128


def images(case, k=0):
    """The u8 images of image set k: [main, neighbour 0, ...], (h, w, 3) or
    (h, w) by the case's channel list."""
    rng = np.random.default_rng([case.seed, k])
    out = []
    for c in case.channels:
        shape = (case.h, case.w, 3) if c == 3 else (case.h, case.w)
        out.append(rng.integers(0, 256, size=shape, dtype=np.uint8))
    if case.bands:
        # Only what the block's own samples read is overwritten, so the patches
        # next to a block keep most of their samples on noise, in both views.
        # (Never a non-zero constant under a textured main patch: the bilinear
        # weights do not sum to exactly 1 in float, norm1 would be rounding
        # noise and the NCC's sign undefined.)
        flat, zero = band_blocks(case)
        x0, y0, x1, y1 = block_pixels(case, flat)
        out[0][y0:y1, x0:x1] = FLAT_BYTE
        for j in range(case.n_subs):
            out[1 + j][block_footprint(case, flat, j)] = FLAT_BYTE
            out[1 + j][block_footprint(case, zero, j)] = 0
    return out


def to_float(img):
    """byte_to_float_image: u8 / 255 in float32."""
    return img.astype(np.float32) / np.float32(255.0)


def problem(oracle, case, k=0, grads=None):
    """oracle.TopologyProblem of image set k (a fresh one: the oracle's calls
    change its surface).  The visibility tests read no gradient plane, so
    zeros stand in without `grads`."""
    g = geometry(case)
    imgs = images(case, k)
    if grads is None:
        grads = [g["views"]["grad"]] * (case.n_subs + 1)
    return oracle.TopologyProblem(g["surf"], [to_float(im) for im in imgs], grads,
                                  g["M"], g["t"], g["main"].flen)


_REPORTS = {}


def report(oracle, case, k=0):
    """TopologyProblem.visibility_report() of image set k, computed once per
    process (read-only)."""
    key = (case.name, k)
    if key not in _REPORTS:
        _REPORTS[key] = problem(oracle, case, k).visibility_report()
    return _REPORTS[key]


_MASKS = {}


def oracle_mask(oracle, case, k=0):
    """orc_topology_subviews' masks of image set k, once per process."""
    key = (case.name, k)
    if key not in _MASKS:
        _MASKS[key] = problem(oracle, case, k).subviews()
    return _MASKS[key]
