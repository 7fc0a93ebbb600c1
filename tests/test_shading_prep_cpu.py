"""CPU checks of the device shading preparation (smvs_ctx_prepare_shading,
lib/stereo_view.cc:64-84): the byte an image float came from is recovered
exactly, the gamma table is the host loop's own expression at the 256 values
an element can take, the host planes are the luminance and the quadratic fit
the kernel reproduces, and the new flags word refuses what it does not know --
none of it needs a device."""
import ctypes as C

import numpy as np


def test_the_byte_comes_back_from_its_float():
    """k -> (float)k / 255.0f -> (int)(v * 255.0f + 0.5f), every operation
    rounded to float32 (the kernel's, with contraction off)."""
    for k in range(256):
        v = np.float32(k) / np.float32(255)
        assert v.dtype == np.float32
        back = v * np.float32(255) + np.float32(0.5)
        assert back.dtype == np.float32
        assert int(back) == k, k


def test_gamma_table_is_the_host_loops_value_for_every_byte():
    """a one-channel view with gamma: the shading plane IS the linear image, so
    pixel k of a row of all 256 bytes holds the host loop's value for byte k
    (bytes 10 and 11 straddle the 0.04045 branch)"""
    from smvs_amd import host
    lut = host.gamma_inv_srgb_lut()
    assert lut.shape == (256,) and lut.dtype == np.float32
    row = np.arange(256, dtype=np.uint8)
    img = np.repeat(row[None, :], 3, axis=0)
    shading, _ = host.shading_planes(img, gamma=True)
    for k in range(256):
        assert shading[1, k] == lut[k], k
    assert np.array_equal(shading, np.repeat(lut[None, :], 3, axis=0))
    # the two branches, from the expression itself
    x = np.arange(256, dtype=np.float32) / np.float32(255)
    assert x[10] <= np.float32(0.04045) < x[11]
    assert np.array_equal(lut[:11], x[:11] / np.float32(12.92))
    assert lut[0] == 0.0 and lut[255] == 1.0 and np.all(np.diff(lut) > 0)
    # without gamma the plane is the image's floats
    plain, _ = host.shading_planes(img, gamma=False)
    assert np.array_equal(plain, np.repeat(x[None, :], 3, axis=0))


def test_host_planes_are_the_luminance_and_the_quadratic_fit(oracle):
    from smvs_amd import host
    rng = np.random.default_rng(64)
    img = rng.integers(0, 256, (19, 37, 3)).astype(np.uint8)
    shading, grad = host.shading_planes(img, gamma=False)
    f = img.astype(np.float32) / np.float32(255)
    want = f[:, :, 0] * np.float32(0.21) + f[:, :, 1] * np.float32(0.72) \
        + f[:, :, 2] * np.float32(0.07)
    assert want.dtype == np.float32
    assert np.array_equal(shading, want)
    assert np.array_equal(grad, oracle.gradients_and_hessian(shading)[0])
    assert np.any(grad != 0) and not np.any(grad[0]) and not np.any(grad[:, 0])


def test_optimize_flags_entry_refuses_an_unknown_flag():
    """before it looks at anything else: no view, no device"""
    from smvs_amd import _capi, host
    hlib = host.load()
    assert hasattr(hlib, "smvs_host_optimize_flags")
    for flags in (2, 3, 1 << 31):
        rc = hlib.smvs_host_optimize_flags(None, None, C.c_int(0), None, None, C.c_int(0),
                                           C.c_int(0), None, None, C.c_uint(flags), None, None,
                                           None)
        assert rc == -1 and b"unknown flag" in hlib.smvs_host_last_error(), flags
    for name in ("smvs_ctx_prepare_shading", "smvs_ctx_download_shading"):
        assert name in _capi.declared_symbols() and hasattr(_capi.load(), name)


def test_scene_flags_word_knows_the_new_bits_and_no_others():
    """bit 3 (device shading preparation) and bit 4 (--gamma-srgb) get past the
    flag check -- the scene directory is what fails -- and the next bit does not"""
    from smvs_amd import host
    hlib = host.load()
    st = host.ReconSettings(b"undistorted", 1.0, 2, 1, 1, 0, 0, 0, 0.0, 0.0, 1, 6, 3, 0, 1, 2,
                            -1, 1700000)

    def call(flags):
        rc = hlib.smvs_host_reconstruct_scene_flags(b"/nonexistent", C.byref(st),
                                                    C.c_uint(flags), None, C.c_int(0), None,
                                                    C.c_int(0), None, None, None, None)
        return rc, hlib.smvs_host_last_error()

    for flags in (8, 16, 8 | 16, 1 | 2 | 8 | 16):
        rc, text = call(flags)
        assert rc != 0 and b"unknown flag" not in text, (flags, text)
    for flags in (32, 8 | 32, 1 << 31):
        rc, text = call(flags)
        assert rc != 0 and b"unknown flag" in text, (flags, text)
