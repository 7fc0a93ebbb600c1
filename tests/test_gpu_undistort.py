"""The undistortion kernel (smvs_undistort_u8, csrc/undistort.hip) against the
numpy restatement (tests/undistort_ref.py) on the case list of
tests/undistort_cases.py, and the COLMAP import that runs it: device and host
form write the same scene, and the rest of the pipeline reads an imported scene
like one written directly.  Every comparison of pixels is array_equal."""
import os

import numpy as np
import pytest

import colmap_helpers as ch
import undistort_cases as uc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import smvs_amd
    if smvs_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on a GPU")
    return smvs_amd


def test_kernel_equals_the_restatement(hip):
    """device.undistort on the whole case list, blank counts included."""
    from smvs_amd import device
    for case in uc.CASES:
        got, blank = device.undistort(uc.image_of(case), case["lens"], case["out_focal"],
                                      case["out_size"], return_blank=True)
        uc.check_case(case, got, blank)


def test_host_mirror_device_form_is_the_same_call(hip):
    """host.undistort(..., device=0) on the whole case list; the blank pointer
    may be NULL; a grey (h, w) array stays (h, w)."""
    import ctypes as C
    from smvs_amd import _capi, device, host
    for case in uc.CASES:
        got, blank = host.undistort(uc.image_of(case), case["lens"], case["out_focal"],
                                    case["out_size"], device=0, return_blank=True)
        uc.check_case(case, got, blank)
    case = [c for c in uc.CASES if c["name"] == "lens_RADIAL_c1"][0]
    a = uc.image_of(case)
    out = np.zeros_like(a)
    L = device.make_lens(case["lens"])
    u8p = C.POINTER(C.c_uint8)
    rc = _capi.load().smvs_undistort_u8(
        C.c_int(0), a.ctypes.data_as(u8p), C.c_int(96), C.c_int(48), C.c_int(1), C.byref(L),
        C.c_float(case["out_focal"]), C.c_int(96), C.c_int(48), out.ctypes.data_as(u8p), None)
    assert rc == 0 and np.array_equal(out, uc.expected(case)[0])
    grey = device.undistort(a[:, :, 0], case["lens"], case["out_focal"])
    assert grey.shape == (48, 96) and np.array_equal(grey, out[:, :, 0])


def test_argument_errors_leave_the_output_untouched(hip):
    """On a machine with a device too, each argument error is SMVS_ERR_INVALID
    and nothing is written."""
    from smvs_amd import _capi
    entry = _capi.load().smvs_undistort_u8
    for name, overrides in uc.ARGUMENT_ERRORS:
        rc, out, blank = uc.call_entry(entry, False, overrides)
        assert rc == -1 and (out == 0xA5).all() and blank == -7, name
    rc, out, blank = uc.call_entry(entry, False, {})
    assert rc == 0 and blank == 0 and (out[36:] == 0xA5).all()
    assert np.array_equal(out[:36], np.arange(36, dtype=np.uint8))


def _tree(root):
    files = {}
    for dirpath, _, names in os.walk(root):
        for n in names:
            p = os.path.join(dirpath, n)
            with open(p, "rb") as f:
                files[os.path.relpath(p, root)] = f.read()
    return files


def test_import_on_the_device_writes_the_host_forms_scene(hip, tmp_path):
    """The 96 x 64 ring with an OPENCV lens on every camera: device=0 and
    device=None write byte-identical scene directories."""
    from smvs_amd import host, mve_scene, synth
    w, h = 96, 64
    inputs = synth.pipeline_inputs("sphere", w, h, 3, flen=128.0 / w, n_features=60)
    params = [120.0, 117.0, 47.0, 33.5, -0.2, 0.05, 0.004, -0.003]
    model = ch.ring_model(inputs["cams"], inputs["features"], "OPENCV", params)
    ch.write_binary(str(tmp_path / "model"), model)
    os.makedirs(str(tmp_path / "images"))
    for k, iid in enumerate(ch.ring_image_ids(4)):
        mve_scene.save_png(str(tmp_path / "images" / model["images"][iid]["name"]),
                           inputs["images"][k])
    reports = {}
    for name, dev in (("host", None), ("device", 0)):
        reports[name] = host.import_colmap(str(tmp_path / "model"), str(tmp_path / "images"),
                                           str(tmp_path / name), zoom=0.8, device=dev)
    a, b = _tree(str(tmp_path / "host")), _tree(str(tmp_path / "device"))
    assert sorted(a) == sorted(b) and len(a) == 2 * 4 + 1
    for name in a:
        assert a[name] == b[name], name
    assert reports["host"]["views"] == reports["device"]["views"]
    assert sum(v["blank_pixels"] for v in reports["device"]["views"]) > 0


def _spread_ring(n=3):
    """The four-view 384 x 256 ring of tests/test_gpu_sgm_photo.py
    (_spread_ring_inputs) with a focal length of 512 pixels, a power of two."""
    from smvs_amd import synth
    w, h, flen, seed = 384, 256, 512.0 / 384.0, 1234
    rng = np.random.default_rng(seed)
    main = synth.ring_cameras(w, h, n, flen=flen)[0]
    subs = [synth.ring_cameras(w, h, n, flen=flen, ring=0.28 - 0.02 * k)[1][k] for k in range(n)]
    scene = synth.SphereScene(seed=seed, px_size=3.0 / (flen * max(w, h)))
    cams = [main] + subs
    images = [synth.render_rgb(scene, c, None) for c in cams]
    xs = rng.uniform(0.05 * w, 0.95 * w, 2000)
    ys = rng.uniform(0.05 * h, 0.95 * h, 2000)
    X, _ = scene.intersect(main.center, synth.pixel_rays(main, xs, ys))
    return dict(cams=cams, images=images, features=X.astype(np.float32))


def test_imported_scene_reconstructs_like_a_written_one(hip, tmp_path):
    """End to end: the ring imported from a PINHOLE model, against a scene
    mve_scene.write_scene wrote from the cameras as read back from the imported
    meta.ini and the same images -- the smvs-sgm and smvs-B0 embeddings of
    reconstruct_scene are equal, which holds poses, bundle and tracks to what the
    rest of the pipeline reads."""
    from smvs_amd import host, mve_scene, synth
    inputs = _spread_ring()
    model = ch.ring_model(inputs["cams"], inputs["features"], "PINHOLE")
    ch.write_binary(str(tmp_path / "model"), model)
    os.makedirs(str(tmp_path / "images"))
    for k, iid in enumerate(ch.ring_image_ids(4)):
        mve_scene.save_png(str(tmp_path / "images" / model["images"][iid]["name"]),
                           inputs["images"][k], filters=(0,))
    imported = str(tmp_path / "imported")
    rep = host.import_colmap(str(tmp_path / "model"), str(tmp_path / "images"), imported,
                             device=0)
    assert rep["views_written"] == 4 and all(v["blank_pixels"] == 0 for v in rep["views"])
    info = host.scene_info(imported)
    assert list(info["present"]) == [1, 1, 1, 1] and info["n_features"] == 2000
    cams = [synth.Camera(info["rot"][k].reshape(3, 3), info["trans"][k], info["flen"][k], 384, 256)
            for k in range(4)]
    for k in range(4):      # the import is the identity on the pixels
        got = host.load_byte_image(os.path.join(imported, "views", "view_%04d.mve" % k,
                                                "undistorted.png"))
        assert np.array_equal(got, inputs["images"][k])
        assert abs(cams[k].flen - inputs["cams"][k].flen) <= 1e-6
        assert np.abs(cams[k].R - inputs["cams"][k].R).max() <= 1e-6
    written = str(tmp_path / "written")
    os.makedirs(written)
    mve_scene.write_scene(written, dict(cams=cams, images=inputs["images"],
                                        features=inputs["features"]))
    for d in (imported, written):
        done, skipped, _ = host.reconstruct_scene(d, view_ids=[0], num_neighbors=3,
                                                  min_neighbors=2, output_scale=2)
        assert done == [0] and skipped == 0
    for name in ("smvs-sgm", "smvs-B0"):
        a = mve_scene.load_mvei(os.path.join(imported, "views", "view_0000.mve", name + ".mvei"))
        b = mve_scene.load_mvei(os.path.join(written, "views", "view_0000.mve", name + ".mvei"))
        assert a.shape == b.shape and np.array_equal(a, b), name
        assert (a > 0).mean() > 0.3, name
