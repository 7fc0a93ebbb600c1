"""CPU checks of the device input scaling (smvs_rescale_half_gaussian,
app/smvsrecon.cc:634-647): the new entries exist, the device entry refuses its
argument errors before it opens a device -- so also on a machine without a GPU
-- and the host function keeps answering the old call form."""
import ctypes as C

import numpy as np
import pytest

_u8p = C.POINTER(C.c_uint8)
INVALID = -1


def _call(lib, w, h, c, halvings, pixels="ok", out="ok", capacity=None, ow="ok", oh="ok"):
    a = np.zeros(max(w * h * c, 1), np.uint8)
    fw, fh = w, h
    for _ in range(max(halvings, 0)):
        fw, fh = (fw + 1) // 2, (fh + 1) // 2
    need = max(fw * fh * max(c, 1), 1)
    buf = np.zeros(need, np.uint8)
    gw, gh = C.c_int(0), C.c_int(0)
    return lib.smvs_rescale_half_gaussian(
        C.c_int(0), a.ctypes.data_as(_u8p) if pixels == "ok" else None, C.c_int(w), C.c_int(h),
        C.c_int(c), C.c_int(halvings), buf.ctypes.data_as(_u8p) if out == "ok" else None,
        C.c_size_t(need if capacity is None else capacity),
        C.byref(gw) if ow == "ok" else None, C.byref(gh) if oh == "ok" else None)


def test_new_entries_exist_and_refuse_bad_arguments_without_a_gpu():
    from smvs_amd import _capi, host
    lib = _capi.load()
    hlib = host.load()
    assert hasattr(lib, "smvs_rescale_half_gaussian")
    assert hasattr(hlib, "smvs_host_rescale_half_size_gaussian_device")
    assert hasattr(hlib, "smvs_host_reconstruct_scene_flags")
    assert "smvs_rescale_half_gaussian" in _capi.declared_symbols()

    def refused(text, *args, **kw):
        assert _call(lib, *args, **kw) == INVALID, (args, kw)
        assert text in lib.smvs_last_error(), (lib.smvs_last_error(), args, kw)

    for which in ("pixels", "out", "ow", "oh"):
        refused(b"null argument", 8, 8, 3, 1, **{which: None})
    for halvings in (0, -1):
        refused(b"halvings", 8, 8, 3, halvings)
    for channels in (0, 5, -2):
        refused(b"channels", 8, 8, channels, 1)
    # the host function's own "image too small": a level narrower or lower than 2
    for w, h, halvings in ((1, 8, 1), (8, 1, 1), (0, 8, 1), (2, 2, 2), (3, 3, 3), (5, 2, 2)):
        refused(b"image too small", w, h, 1, halvings)
    # 8 x 6 x 3, one halving: 4 x 3 x 3 = 36 bytes
    refused(b"output buffer too small", 8, 6, 3, 1, capacity=35)
    refused(b"output buffer too small", 8, 6, 3, 2, capacity=11)
    # the host mirror hands the same refusals on (and its own for a bad call)
    a = np.zeros((3, 3, 1), np.uint8)
    with pytest.raises(_capi.SmvsError, match="image too small"):
        host.rescale_half_size_gaussian(a, halvings=3, device=0)
    with pytest.raises(_capi.SmvsError, match="channels"):
        host.rescale_half_size_gaussian(np.zeros((4, 4, 5), np.uint8), device=0)
    with pytest.raises(_capi.SmvsError, match="halvings"):
        host.rescale_half_size_gaussian(np.zeros((4, 4, 3), np.uint8), halvings=0, device=0)


def test_scene_flags_entry_refuses_an_unknown_flag():
    from smvs_amd import host
    hlib = host.load()
    st = host.ReconSettings(b"undistorted", 1.0, 2, 0, 1, 0, 0, 0, 0.0, 0.0, 1, 6, 3, 0, 1, 2,
                            -1, 1700000)
    rc = hlib.smvs_host_reconstruct_scene_flags(b"/nonexistent", C.byref(st), C.c_uint(4), None,
                                                C.c_int(0), None, C.c_int(0), None, None, None,
                                                None)
    assert rc != 0 and b"unknown flag" in hlib.smvs_host_last_error()


@pytest.mark.parametrize("shape", [(7, 9, 3), (2, 2, 1), (33, 20, 4), (16, 31)])
def test_old_call_form_still_equals_the_oracle(oracle, shape):
    from smvs_amd import host
    rng = np.random.default_rng(sum(shape))
    a = rng.integers(0, 256, shape).astype(np.uint8)
    got = host.rescale_half_size_gaussian(a)
    want = oracle.rescale_half_size_gaussian(a)
    assert got.shape == want.shape and np.array_equal(got, want)
    # the host chain (no device): the function applied repeatedly
    if min(shape[:2]) >= 4:
        twice = host.rescale_half_size_gaussian(a, halvings=2)
        assert np.array_equal(twice, oracle.rescale_half_size_gaussian(want))
