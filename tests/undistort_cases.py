"""The case list of the undistortion tests, shared by the CPU tests (host form)
and the GPU tests (kernel): the smallest shapes at which the kernel can go
wrong, with the restatement's answer computed once per case.

The kernel's tile (csrc/undistort.hip) is UND_TX x UND_TY = 64 x 16 output
pixels per workgroup, a lane per aligned dword of an output row."""
import numpy as np

import undistort_ref as ref

TILE_X, TILE_Y = 64, 16

# (width, height): tiny images; 37 x 23, whose 3-channel rows are 111 bytes, so
# that no row but the first starts dword-aligned; exactly one tile; one tile
# plus one pixel in x, in y, in both; several tiles with ragged edges
SIZES = [(1, 1), (2, 2), (3, 5), (37, 23),
         (TILE_X, TILE_Y), (TILE_X + 1, TILE_Y), (TILE_X, TILE_Y + 1),
         (TILE_X + 1, TILE_Y + 1), (130, 20), (257, 33)]
CHANNELS = [1, 3, 4]
CONTENTS = ["random", "white", "checker", "ramp"]


def make_image(width, height, channels, content, seed=0):
    if content == "random":
        rng = np.random.default_rng(1000 * width + 10 * height + channels + seed)
        a = rng.integers(0, 256, (height, width, channels), dtype=np.uint8)
    elif content == "white":
        a = np.full((height, width, channels), 255, np.uint8)
    elif content == "checker":      # period 1: bilinear sums near .5
        yy, xx = np.mgrid[0:height, 0:width]
        a = np.repeat((((xx + yy) & 1) * 255).astype(np.uint8)[:, :, None], channels, axis=2)
    elif content == "ramp":
        yy, xx = np.mgrid[0:height, 0:width]
        a = np.stack([((3 * xx + 5 * yy + 41 * ch) & 255).astype(np.uint8)
                      for ch in range(channels)], axis=2)
    else:
        raise ValueError(content)
    return np.ascontiguousarray(a)


def size_lens(width, height):
    """An OPENCV lens in proportion to the image: every term of the model at
    work, most of the output inside, some of it blank."""
    m = float(max(width, height))
    return ref.lens_dict(0.83 * m, 0.79 * m, 0.5 * width + 0.3, 0.5 * height - 0.2,
                         -0.25, 0.08, 0.01, -0.02)


# out_focal of the size cases over the lens's fx: zoomed out, so that the border
# of the output is blank and the rest is inside
SIZE_ZOOM = 0.7


def identity_lens(width, height):
    return ref.lens_dict(64.0, 64.0, 0.5 * width, 0.5 * height)


# The lenses on 96 x 48 with the blank counts the restatement gives
# (name, lens, out_focal, out_size, blank pixels)
LENS_CASES = [
    ("PINHOLE", ref.lens_dict(80, 70, 50.25, 22.5), 80.0, None, 144),
    ("SIMPLE_RADIAL", ref.lens_dict(80, 80, 48, 24, -0.3), 80.0, None, 0),
    ("RADIAL", ref.lens_dict(80, 80, 48, 24, 0.2, 0.05), 80.0, None, 600),
    ("OPENCV", ref.lens_dict(82, 79, 47, 25, -0.25, 0.08, 0.01, -0.02), 82.0, None, 0),
    ("SIMPLE_RADIAL_focal56", ref.lens_dict(80, 80, 48, 24, -0.3), 56.0, None, 1748),
    ("SIMPLE_RADIAL_focal120", ref.lens_dict(80, 80, 48, 24, -0.3), 120.0, None, 0),
    ("SIMPLE_RADIAL_out120x70", ref.lens_dict(80, 80, 48, 24, -0.3), 80.0, (120, 70), 2544),
    ("cx4000", ref.lens_dict(80, 80, 4000, 24), 80.0, None, 4608),
]


def _cases():
    out = []
    for (w, h) in SIZES:
        for c in CHANNELS:
            for content in CONTENTS:
                out.append(dict(name="size_%dx%dx%d_%s" % (w, h, c, content), width=w,
                                height=h, channels=c, content=content, lens=size_lens(w, h),
                                out_focal=SIZE_ZOOM * size_lens(w, h)["fx"], out_size=None,
                                blank=None,
                                identity=False))
            out.append(dict(name="identity_%dx%dx%d" % (w, h, c), width=w, height=h,
                            channels=c, content="random", lens=identity_lens(w, h),
                            out_focal=64.0, out_size=None, blank=0, identity=True))
    for name, lens, focal, out_size, blank in LENS_CASES:
        for c in CHANNELS:
            out.append(dict(name="lens_%s_c%d" % (name, c), width=96, height=48, channels=c,
                            content="random", lens=lens, out_focal=focal, out_size=out_size,
                            blank=blank, identity=False))
    return out


CASES = _cases()
_cache = {}


def image_of(case):
    return make_image(case["width"], case["height"], case["channels"], case["content"])


def expected(case):
    """(output, blank pixels) of the restatement; computed once, read-only."""
    if case["name"] not in _cache:
        out, blank = ref.undistort(image_of(case), case["lens"], case["out_focal"],
                                   case["out_size"])
        out.setflags(write=False)
        _cache[case["name"]] = (out, blank)
    return _cache[case["name"]]


def check_case(case, got, got_blank):
    """Every comparison is array_equal: nothing excluded, no tolerance."""
    want, want_blank = expected(case)
    assert got.shape == want.shape, case["name"]
    assert np.array_equal(got, want), case["name"]
    assert got_blank == want_blank, (case["name"], got_blank, want_blank)
    if case["blank"] is not None:
        assert got_blank == case["blank"], (case["name"], got_blank, case["blank"])
    if case["identity"]:
        assert np.array_equal(got, image_of(case)), case["name"]
    if case["name"].startswith("lens_cx4000"):
        assert not got.any(), case["name"]


# Argument errors of smvs_undistort_u8 / smvs_host_undistort_u8 on a 4 x 3 x 3
# image: (name, overrides) -- every one returns SMVS_ERR_INVALID and leaves the
# output buffer untouched
ARGUMENT_ERRORS = [
    ("null_pixels", dict(pixels=None)),
    ("null_lens", dict(lens=None)),
    ("null_out", dict(out=None)),
    ("channels_0", dict(channels=0)),
    ("channels_5", dict(channels=5)),
    ("width_0", dict(width=0)),
    ("height_0", dict(height=0)),
    ("height_negative", dict(height=-3)),
    ("out_width_0", dict(out_width=0)),
    ("out_height_0", dict(out_height=0)),
    ("out_focal_0", dict(out_focal=0.0)),
    ("out_focal_negative", dict(out_focal=-5.0)),
    ("out_focal_nan", dict(out_focal=float("nan"))),
] + [("lens_%s_%s" % (k, n), dict(lens_field=(k, v)))
     for k in ref.LENS_KEYS for n, v in (("nan", float("nan")), ("inf", float("inf")))]


def call_entry(entry, is_host, overrides):
    """One call of smvs_undistort_u8 / smvs_host_undistort_u8 on a 4 x 3 x 3 image
    with the overrides of undistort_cases.ARGUMENT_ERRORS -> (rc, output buffer)."""
    import ctypes as C
    from smvs_amd.device import Lens
    u8p = C.POINTER(C.c_uint8)
    a = np.arange(36, dtype=np.uint8)
    out = np.full(4 * 3 * 3 + 64, 0xA5, np.uint8)
    lens = Lens(4.0, 4.0, 2.0, 1.5, 0.0, 0.0, 0.0, 0.0)
    if "lens_field" in overrides:
        setattr(lens, *overrides["lens_field"])
    v = dict(pixels=a.ctypes.data_as(u8p), width=4, height=3, channels=3, lens=C.byref(lens),
             out_focal=4.0, out_width=4, out_height=3, out=out.ctypes.data_as(u8p))
    v.update({k: x for k, x in overrides.items() if k != "lens_field"})
    blank = C.c_int64(-7)
    head = [v["pixels"], C.c_int(v["width"]), C.c_int(v["height"]), C.c_int(v["channels"]),
            v["lens"], C.c_float(v["out_focal"]), C.c_int(v["out_width"]),
            C.c_int(v["out_height"])]
    if is_host:
        rc = entry(*head, C.c_int(-1), v["out"], C.byref(blank))
    else:
        rc = entry(C.c_int(0), *head, v["out"], C.byref(blank))
    return rc, out, blank.value
