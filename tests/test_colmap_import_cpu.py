"""CPU checks of the COLMAP importer (csrc/host/colmap_io.h): the host form of
the undistortion against the numpy restatement on the whole case list, the
argument errors of both entries, the model reader on text and binary files and
on broken ones, and the import of a synthetic ring as an MVE scene.  Every
comparison of pixels is array_equal."""
import os

import numpy as np
import pytest

import colmap_helpers as ch
import undistort_cases as uc


@pytest.fixture(scope="module")
def host():
    from smvs_amd import build as hip_build, host
    hip_build.build()
    host.load()
    return host


def test_entries_exist(host):
    from smvs_amd import _capi, device
    assert "smvs_undistort_u8" in _capi.declared_symbols()
    assert hasattr(_capi.load(), "smvs_undistort_u8")
    for name in ("smvs_host_import_colmap", "smvs_host_read_colmap_model",
                 "smvs_host_undistort_u8"):
        assert hasattr(host.load(), name), name
    for name in ("import_colmap", "read_colmap_model", "undistort"):
        assert callable(getattr(host, name))
    assert callable(device.undistort)


def test_host_form_equals_the_restatement(host):
    """The whole case list: sizes x channels x contents with an OPENCV lens, the
    identity at every size, the eight lenses on 96 x 48 with their blank counts."""
    assert len(uc.CASES) == len(uc.SIZES) * len(uc.CHANNELS) * (len(uc.CONTENTS) + 1) \
        + len(uc.LENS_CASES) * len(uc.CHANNELS)
    for case in uc.CASES:
        got, blank = host.undistort(uc.image_of(case), case["lens"], case["out_focal"],
                                    case["out_size"], return_blank=True)
        uc.check_case(case, got, blank)


def test_case_list_reaches_what_it_names():
    """The size cases are not all-inside or all-blank, and the checkerboard does
    produce sums near .5."""
    some_blank = some_inside = 0
    for case in uc.CASES:
        want, blank = uc.expected(case)
        if case["name"].startswith("size_") and case["width"] >= 37:
            some_blank += blank > 0
            some_inside += blank < want.shape[0] * want.shape[1]
    assert some_blank > 0 and some_inside > 0
    case = [c for c in uc.CASES if c["name"] == "size_130x20x1_checker"][0]
    want, _ = uc.expected(case)
    assert ((want > 100) & (want < 156)).sum() > 50


@pytest.mark.parametrize("which", ["device_entry", "host_entry"])
def test_argument_errors(host, which):
    """Each one is SMVS_ERR_INVALID (-1) before any device call -- so also without
    a device -- and the output buffer is untouched."""
    from smvs_amd import _capi
    entry = _capi.load().smvs_undistort_u8 if which == "device_entry" \
        else host.load().smvs_host_undistort_u8
    assert len(uc.ARGUMENT_ERRORS) == 13 + 16
    for name, overrides in uc.ARGUMENT_ERRORS:
        rc, out, blank = uc.call_entry(entry, which == "host_entry", overrides)
        assert rc == -1, name
        assert (out == 0xA5).all(), name
        assert blank == -7, name
    if which == "host_entry":      # the same call without an override is fine
        rc, out, blank = uc.call_entry(entry, True, {})
        assert rc == 0 and blank == 0 and (out[36:] == 0xA5).all()
        assert np.array_equal(out[:36], np.arange(36, dtype=np.uint8))
    with pytest.raises(Exception):
        host.undistort(np.zeros((3, 4, 5), np.uint8), dict(f=4, cx=2, cy=1.5), 4.0)


@pytest.fixture(scope="module")
def fixtures(tmp_path_factory):
    return ch.write_fixtures(str(tmp_path_factory.mktemp("colmap_fixtures")))


def test_text_and_binary_read_back_equal(host, fixtures):
    model = ch.base_model()
    (text_dir, ok_t, _), (bin_dir, ok_b, _) = fixtures[0], fixtures[1]
    assert ok_t and ok_b
    assert "\n\n" in open(os.path.join(text_dir, "images.txt")).read()   # the empty line
    got_t = host.read_colmap_model(text_dir)
    got_b = host.read_colmap_model(bin_dir)
    assert got_t["binary"] is False and got_b["binary"] is True
    ch.assert_models_equal(got_t, model)
    ch.assert_models_equal(got_b, model)
    assert got_t["images"][12]["name"] == "dir with space/img 12.png"
    assert len(got_t["images"][3]["point3D_ids"]) == 0
    assert list(got_b["images"][12]["point3D_ids"]) == [9, -1]


def test_binary_is_preferred_only_when_complete(host, tmp_path):
    """.bin if all three are there, else .txt."""
    model = ch.base_model()
    d = str(tmp_path / "both")
    ch.write_text(d, model)
    other = ch.base_model()
    other["cameras"][2]["params"] = np.array([71.0, 32.0, 24.0, -0.1])
    ch.write_binary(d, other)
    assert host.read_colmap_model(d)["cameras"][2]["params"][0] == 71.0
    os.remove(os.path.join(d, "points3D.bin"))
    assert host.read_colmap_model(d)["cameras"][2]["params"][0] == 70.0


def test_reader_errors(host, fixtures):
    """Unsupported models are named; truncated and inconsistent files are errors
    that name the file, never a crash or a silent success."""
    from smvs_amd._capi import SmvsError
    bad = [f for f in fixtures if not f[1]]
    assert len(bad) > 50
    assert sum("unsupported_" in f[0] for f in bad) == 2 * len(ch.UNSUPPORTED)
    for path, _, needle in bad:
        with pytest.raises(SmvsError) as e:
            host.read_colmap_model(path)
        if needle is not None:
            assert needle in str(e.value), (path, str(e.value))
    for path, _, _ in bad:
        if "unsupported_" in path:
            with pytest.raises(SmvsError) as e:
                host.read_colmap_model(path)
            assert "camera 7" in str(e.value) and "not supported" in str(e.value)


# ------------------------------------------------------------------ the ring
W, H, F = 96, 64, 128.0     # f a power of two: the import is the identity


@pytest.fixture(scope="module")
def ring(tmp_path_factory):
    """synth cameras on a ring, rendered at 96 x 64, as a COLMAP model (text) and
    PNG files; IMAGE_IDs 3, 5, 8, 10."""
    from smvs_amd import synth, mve_scene
    root = str(tmp_path_factory.mktemp("ring"))
    inputs = synth.pipeline_inputs("sphere", W, H, 3, flen=F / max(W, H), n_features=60)
    cams, images = inputs["cams"], inputs["images"]
    model = ch.ring_model(cams, inputs["features"])
    ch.write_text(os.path.join(root, "model"), model)
    os.makedirs(os.path.join(root, "images"))
    for im, img in zip([model["images"][i] for i in ch.ring_image_ids(4)], images):
        mve_scene.save_png(os.path.join(root, "images", im["name"]), img)
    return dict(root=root, model_dir=os.path.join(root, "model"),
                image_dir=os.path.join(root, "images"), cams=cams, images=images,
                features=inputs["features"], model=model)


def test_import_ring_is_the_scene_of_the_synth_cameras(host, ring, tmp_path):
    from smvs_amd import mve_scene
    scene = str(tmp_path / "scene")
    rep = host.import_colmap(ring["model_dir"], ring["image_dir"], scene)
    assert rep["num_views"] == 4 and rep["views_written"] == 4
    assert [v["view_id"] for v in rep["views"]] == [0, 1, 2, 3]
    assert [v["image_id"] for v in rep["views"]] == ch.ring_image_ids(4)
    assert [v["name"] for v in rep["views"]] == ["ring_%02d.png" % k for k in range(4)]
    assert all(v["blank_pixels"] == 0 and v["channels"] == 3 for v in rep["views"])
    assert (rep["points_kept"], rep["points_dropped"]) == (60, 0)
    assert (rep["track_elements_kept"], rep["track_elements_dropped"]) == (240, 0)
    info = host.scene_info(scene)
    assert list(info["present"]) == [1, 1, 1, 1] and info["n_features"] == 60
    assert list(info["width"]) == [W] * 4 and list(info["height"]) == [H] * 4
    for k, cam in enumerate(ring["cams"]):
        assert abs(info["flen"][k] - cam.flen) <= 1e-6
        assert np.abs(info["rot"][k].reshape(3, 3) - cam.R).max() <= 1e-6
        assert np.abs(info["trans"][k] - cam.t).max() <= 1e-6
        png = os.path.join(scene, "views", "view_%04d.mve" % k, "undistorted.png")
        assert np.array_equal(mve_scene.load_png(png), ring["images"][k])
        assert np.array_equal(host.load_byte_image(png), ring["images"][k])
        meta = open(os.path.join(scene, "views", "view_%04d.mve" % k, "meta.ini")).read()
        assert "pixel_aspect = 1\n" in meta and "principal_point = 0.5 0.5\n" in meta
        assert "id = %d\nname = ring_%02d.png\n" % (k, k) in meta
    # the bundle as the rest of the pipeline reads it: view selection
    bcams, feats, cols, refs = ch.read_bundle(os.path.join(scene, "synth_0.out"))
    assert len(bcams) == 4 and np.array_equal(feats, ring["features"])
    assert (cols == 255).all()
    assert all(r == [(v, i) for v in range(4)] for i, r in enumerate(refs))
    for k in range(4):
        assert abs(bcams[k][0] - info["flen"][k]) <= 1e-7
    imported = dict(views=[dict(id=k, flen=info["flen"][k], rot=info["rot"][k],
                                trans=info["trans"][k], width=W, height=H) for k in range(4)],
                    features=feats, refs=[[v for v, _ in r] for r in refs])
    synth_scene = dict(views=[dict(id=k, flen=c.flen, rot=c.R, trans=c.t, width=W, height=H)
                              for k, c in enumerate(ring["cams"])],
                       features=ring["features"], refs=[list(range(4))] * 60)
    for view in range(4):
        assert host.select_neighbors(imported, view, num_neighbors=3) \
            == host.select_neighbors(synth_scene, view, num_neighbors=3)


def test_import_containers_and_grey(host, ring, tmp_path):
    """mvei holds the same bytes; a grey image stays grey."""
    from smvs_amd import mve_scene
    scene = str(tmp_path / "scene_mvei")
    host.import_colmap(ring["model_dir"], ring["image_dir"], scene, container="mvei", threads=1)
    for k in range(4):
        d = os.path.join(scene, "views", "view_%04d.mve" % k)
        assert not os.path.exists(os.path.join(d, "undistorted.png"))
        assert np.array_equal(mve_scene.load_mvei(os.path.join(d, "undistorted.mvei")),
                              ring["images"][k])
    grey_dir = str(tmp_path / "grey")
    os.makedirs(grey_dir)
    for k in range(4):
        mve_scene.save_png(os.path.join(grey_dir, "ring_%02d.png" % k), ring["images"][k][:, :, 1])
    scene = str(tmp_path / "scene_grey")
    rep = host.import_colmap(ring["model_dir"], grey_dir, scene)
    assert all(v["channels"] == 1 for v in rep["views"])
    got = host.load_byte_image(os.path.join(scene, "views", "view_0002.mve", "undistorted.png"))
    assert np.array_equal(got, ring["images"][2][:, :, 1])


def test_import_with_a_lens_matches_the_restatement(host, ring, tmp_path):
    """An OPENCV camera, zoom and an output size of its own: the embedding is the
    restatement of the rendered image, the report counts its blank pixels, flen is
    out_focal / max(out size)."""
    import undistort_ref as ref
    params = [120.0, 117.0, 47.0, 33.5, -0.2, 0.05, 0.004, -0.003]
    model = ch.ring_model(ring["cams"], ring["features"], "OPENCV", params)
    model_dir = str(tmp_path / "model")
    ch.write_binary(model_dir, model)
    scene = str(tmp_path / "scene")
    rep = host.import_colmap(model_dir, ring["image_dir"], scene, zoom=0.75, out_size=(80, 50),
                             threads=3)
    lens = ref.lens_dict(*params)
    info = host.scene_info(scene)
    for k in range(4):
        want, blank = ref.undistort(ring["images"][k], lens, np.float32(0.75) * np.float32(120.0),
                                    (80, 50))
        got = host.load_byte_image(os.path.join(scene, "views", "view_%04d.mve" % k,
                                                "undistorted.png"))
        assert np.array_equal(got, want)
        assert rep["views"][k]["blank_pixels"] == blank
        assert (rep["views"][k]["width"], rep["views"][k]["height"]) == (80, 50)
        assert info["flen"][k] == np.float32(90.0) / np.float32(80.0)
    assert sum(v["blank_pixels"] for v in rep["views"]) > 0


def test_import_refusals(host, ring, tmp_path):
    from smvs_amd import mve_scene
    from smvs_amd._capi import SmvsError
    scene = str(tmp_path / "scene")
    host.import_colmap(ring["model_dir"], ring["image_dir"], scene)
    with pytest.raises(SmvsError, match="views"):
        host.import_colmap(ring["model_dir"], ring["image_dir"], scene)
    host.import_colmap(ring["model_dir"], ring["image_dir"], scene, overwrite=True)
    # an image whose size differs from its camera's, one that cannot be decoded,
    # one that is missing: errors that name the file
    other = str(tmp_path / "images")
    os.makedirs(other)
    for k in range(4):
        mve_scene.save_png(os.path.join(other, "ring_%02d.png" % k), ring["images"][k])
    mve_scene.save_png(os.path.join(other, "ring_01.png"), ring["images"][1][:, :-1])
    with pytest.raises(SmvsError, match="ring_01.png"):
        host.import_colmap(ring["model_dir"], other, str(tmp_path / "s2"))
    with open(os.path.join(other, "ring_01.png"), "wb") as f:
        f.write(b"not a png")
    with pytest.raises(SmvsError, match="ring_01.png"):
        host.import_colmap(ring["model_dir"], other, str(tmp_path / "s3"))
    os.remove(os.path.join(other, "ring_01.png"))
    with pytest.raises(SmvsError, match="ring_01.png"):
        host.import_colmap(ring["model_dir"], other, str(tmp_path / "s4"))
    for bad in (dict(threads=0), dict(threads=17), dict(zoom=0.0), dict(out_size=(0, 5)),
                dict(view_ids=[4]), dict(view_ids=[-1])):
        with pytest.raises(SmvsError):
            host.import_colmap(ring["model_dir"], ring["image_dir"], str(tmp_path / "s5"), **bad)
    with pytest.raises(ValueError):
        host.import_colmap(ring["model_dir"], ring["image_dir"], str(tmp_path / "s6"),
                           container="jpg")


def test_view_ids_restrict_the_views(host, ring, tmp_path):
    """Views 0 and 2 only: the others are holes of the view list, their track
    elements are dropped and counted; a point only they see is dropped."""
    model = ch.ring_model(ring["cams"], ring["features"])
    ids = ch.ring_image_ids(4)
    model["points3D"][7]["image_ids"] = np.asarray([ids[1], ids[3]], np.uint32)
    model["points3D"][7]["point2D_idxs"] = np.asarray([6, 6], np.uint32)
    model_dir = str(tmp_path / "model")
    ch.write_binary(model_dir, model)
    scene = str(tmp_path / "scene")
    rep = host.import_colmap(model_dir, ring["image_dir"], scene, view_ids=[2, 0])
    assert [v["view_id"] for v in rep["views"]] == [0, 2]
    assert [v["image_id"] for v in rep["views"]] == [ids[0], ids[2]]
    assert rep["num_views"] == 4 and rep["views_written"] == 2
    assert (rep["points_kept"], rep["points_dropped"]) == (59, 1)
    assert (rep["track_elements_kept"], rep["track_elements_dropped"]) == (118, 120)
    info = host.scene_info(scene)
    assert list(info["present"]) == [1, 0, 1] and info["n_features"] == 59
    _, feats, _, refs = ch.read_bundle(os.path.join(scene, "synth_0.out"))
    assert all([v for v, _ in r] == [0, 2] for r in refs)
    assert np.array_equal(feats, np.delete(ring["features"], 6, axis=0))
    assert sorted(os.listdir(os.path.join(scene, "views"))) == ["view_0000.mve", "view_0002.mve"]
