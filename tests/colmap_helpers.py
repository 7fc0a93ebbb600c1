"""Test helpers of the COLMAP importer: a small writer of COLMAP models as text
and as binary (tests/golden/COLMAP.md C1-C9 [COLMAP-unverified]), the model of a
synth ring, and a reader of synth_0.out.  Models are dicts in the form
smvs_amd.host.read_colmap_model returns."""
import os
import struct

import numpy as np

MODEL_IDS = {"SIMPLE_PINHOLE": 0, "PINHOLE": 1, "SIMPLE_RADIAL": 2, "RADIAL": 3, "OPENCV": 4,
             "OPENCV_FISHEYE": 5, "FULL_OPENCV": 6, "FOV": 7, "SIMPLE_RADIAL_FISHEYE": 8,
             "RADIAL_FISHEYE": 9, "THIN_PRISM_FISHEYE": 10}
UNSUPPORTED = {"OPENCV_FISHEYE": 8, "FULL_OPENCV": 12, "FOV": 5, "SIMPLE_RADIAL_FISHEYE": 4,
               "RADIAL_FISHEYE": 5, "THIN_PRISM_FISHEYE": 12}
NO_POINT = 0xFFFFFFFFFFFFFFFF


def _g(v):
    return "%.17g" % float(v)


def write_text(model_dir, model, comments=True):
    """cameras.txt, images.txt, points3D.txt in the dicts' order (C3-C5)."""
    os.makedirs(model_dir, exist_ok=True)
    with open(os.path.join(model_dir, "cameras.txt"), "w") as f:
        if comments:
            f.write("# Camera list with one line of data per camera:\n"
                    "#   CAMERA_ID, MODEL, WIDTH, HEIGHT, PARAMS[]\n"
                    "# Number of cameras: %d\n" % len(model["cameras"]))
        for cid, c in model["cameras"].items():
            f.write("%d %s %d %d %s\n" % (cid, c["model"], c["width"], c["height"],
                                          " ".join(_g(p) for p in c["params"])))
    with open(os.path.join(model_dir, "images.txt"), "w") as f:
        if comments:
            f.write("# Image list with two lines of data per image:\n"
                    "#   IMAGE_ID, QW, QX, QY, QZ, TX, TY, TZ, CAMERA_ID, NAME\n"
                    "#   POINTS2D[] as (X, Y, POINT3D_ID)\n")
        for iid, im in model["images"].items():
            f.write("%d %s %s %d %s\n" % (iid, " ".join(_g(v) for v in im["q"]),
                                          " ".join(_g(v) for v in im["t"]), im["camera_id"],
                                          im["name"]))
            # (an image without 2D points has an EMPTY second line)
            f.write(" ".join("%s %s %d" % (_g(x), _g(y), p)
                             for (x, y), p in zip(im["xys"], im["point3D_ids"])) + "\n")
    with open(os.path.join(model_dir, "points3D.txt"), "w") as f:
        if comments:
            f.write("# 3D point list with one line of data per point:\n"
                    "#   POINT3D_ID, X, Y, Z, R, G, B, ERROR, TRACK[] as (IMAGE_ID, POINT2D_IDX)\n")
        for pid, p in model["points3D"].items():
            track = " ".join("%d %d" % (i, k) for i, k in zip(p["image_ids"], p["point2D_idxs"]))
            f.write(("%d %s %d %d %d %s %s" % (pid, " ".join(_g(v) for v in p["xyz"]),
                                               p["rgb"][0], p["rgb"][1], p["rgb"][2],
                                               _g(p["error"]), track)).rstrip() + "\n")


def binary_sections(model):
    """-> (cameras.bin, images.bin, points3D.bin) bytes and, per file, the byte
    offsets at which a record starts or ends (C6-C8)."""
    cams = [struct.pack("<Q", len(model["cameras"]))]
    for cid, c in model["cameras"].items():
        cams.append(struct.pack("<IiQQ", cid, MODEL_IDS[c["model"]], c["width"], c["height"])
                    + struct.pack("<%dd" % len(c["params"]), *[float(p) for p in c["params"]]))
    imgs = [struct.pack("<Q", len(model["images"]))]
    for iid, im in model["images"].items():
        rec = struct.pack("<I4d3dI", iid, *[float(v) for v in im["q"]],
                          *[float(v) for v in im["t"]], im["camera_id"])
        rec += im["name"].encode() + b"\0" + struct.pack("<Q", len(im["point3D_ids"]))
        for (x, y), p in zip(im["xys"], im["point3D_ids"]):
            rec += struct.pack("<ddQ", float(x), float(y), NO_POINT if p < 0 else int(p))
        imgs.append(rec)
    pts = [struct.pack("<Q", len(model["points3D"]))]
    for pid, p in model["points3D"].items():
        rec = struct.pack("<Q3d3BdQ", pid, *[float(v) for v in p["xyz"]],
                          *[int(v) for v in p["rgb"]], float(p["error"]), len(p["image_ids"]))
        for i, k in zip(p["image_ids"], p["point2D_idxs"]):
            rec += struct.pack("<II", int(i), int(k))
        pts.append(rec)
    files, bounds = [], []
    for parts in (cams, imgs, pts):
        files.append(b"".join(parts))
        bounds.append(list(np.cumsum([len(x) for x in parts])))
    return files, bounds


BIN_NAMES = ("cameras.bin", "images.bin", "points3D.bin")


def write_binary(model_dir, model):
    os.makedirs(model_dir, exist_ok=True)
    files, _ = binary_sections(model)
    for name, data in zip(BIN_NAMES, files):
        with open(os.path.join(model_dir, name), "wb") as f:
            f.write(data)


def assert_models_equal(got, want):
    assert sorted(got["cameras"]) == sorted(want["cameras"])
    for cid, c in want["cameras"].items():
        g = got["cameras"][cid]
        assert (g["model"], g["width"], g["height"]) == (c["model"], c["width"], c["height"])
        assert np.array_equal(np.asarray(g["params"], float), np.asarray(c["params"], float))
    assert sorted(got["images"]) == sorted(want["images"])
    for iid, im in want["images"].items():
        g = got["images"][iid]
        assert g["name"] == im["name"] and g["camera_id"] == im["camera_id"], iid
        assert np.array_equal(g["q"], np.asarray(im["q"], float)), iid
        assert np.array_equal(g["t"], np.asarray(im["t"], float)), iid
        assert np.array_equal(np.asarray(g["xys"], float).reshape(-1, 2),
                              np.asarray(im["xys"], float).reshape(-1, 2)), iid
        assert np.array_equal(g["point3D_ids"], np.asarray(im["point3D_ids"], np.int64)), iid
    assert sorted(got["points3D"]) == sorted(want["points3D"])
    for pid, p in want["points3D"].items():
        g = got["points3D"][pid]
        assert np.array_equal(g["xyz"], np.asarray(p["xyz"], float)), pid
        assert np.array_equal(g["rgb"], np.asarray(p["rgb"], np.uint8)), pid
        assert g["error"] == float(p["error"]), pid
        assert np.array_equal(g["image_ids"], np.asarray(p["image_ids"], np.uint32)), pid
        assert np.array_equal(g["point2D_idxs"], np.asarray(p["point2D_idxs"], np.uint32)), pid


def rotation_to_quaternion(R):
    """(w, x, y, z) of a rotation matrix (world -> camera, as COLMAP stores it)."""
    R = np.asarray(R, float)
    tr = np.trace(R)
    if tr > 0:
        s = 2.0 * np.sqrt(1.0 + tr)
        q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = 2.0 * np.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k])
        q = [0.0] * 4
        q[0] = (R[k, j] - R[j, k]) / s
        q[1 + i] = 0.25 * s
        q[1 + j] = (R[j, i] + R[i, j]) / s
        q[1 + k] = (R[k, i] + R[i, k]) / s
    return np.asarray(q, float)


# IMAGE_IDs of a ring's views 0, 1, 2, ...: they start above 1 and have gaps
def ring_image_ids(n):
    return [3 + 2 * i + (i // 2) for i in range(n)]


def ring_model(cams, features, camera_model="PINHOLE", params=None, names=None):
    """The COLMAP model of synth cameras (all of one size, one COLMAP camera):
    image k of the ring has IMAGE_ID ring_image_ids[k] and is written out of
    order; every feature is seen by every image, as point2D `feature index`."""
    n = len(cams)
    w, h = cams[0].width, cams[0].height
    f = cams[0].flen * max(w, h)
    if params is None:
        params = {"PINHOLE": [f, f, 0.5 * w, 0.5 * h], "SIMPLE_PINHOLE": [f, 0.5 * w, 0.5 * h]}[
            camera_model]
    ids = ring_image_ids(n)
    names = names or ["ring_%02d.png" % k for k in range(n)]
    feats = np.asarray(features, np.float32)
    images = {}
    for k in reversed(range(n)):
        images[ids[k]] = dict(q=rotation_to_quaternion(cams[k].R), t=np.asarray(cams[k].t, float),
                              camera_id=5, name=names[k],
                              xys=np.zeros((len(feats), 2)),
                              point3D_ids=np.arange(len(feats), dtype=np.int64) + 1)
    points = {}
    for i in reversed(range(len(feats))):
        points[i + 1] = dict(xyz=feats[i].astype(float), rgb=np.array([255, 255, 255], np.uint8),
                             error=0.5, image_ids=np.asarray(ids, np.uint32),
                             point2D_idxs=np.full(n, i, np.uint32))
    return dict(cameras={5: dict(model=camera_model, width=w, height=h,
                                 params=np.asarray(params, float))},
                images=images, points3D=points)


def read_bundle(path):
    """synth_0.out (M28) -> (cameras [(flen, R (3, 3), t)], features (F, 3), colours
    (F, 3), refs [[(view id, feature id)]])."""
    tok = open(path).read().split()
    assert tok[:2] == ["drews", "1.0"]
    nc, nf = int(tok[2]), int(tok[3])
    at = 4
    cams = []
    for _ in range(nc):
        v = [float(x) for x in tok[at:at + 15]]
        at += 15
        cams.append((v[0], np.asarray(v[3:12]).reshape(3, 3), np.asarray(v[12:15])))
    feats, cols, refs = [], [], []
    for _ in range(nf):
        feats.append([float(x) for x in tok[at:at + 3]])
        cols.append([int(x) for x in tok[at + 3:at + 6]])
        m = int(tok[at + 6])
        at += 7
        refs.append([(int(tok[at + 3 * k]), int(tok[at + 3 * k + 1])) for k in range(m)])
        at += 3 * m
    assert at == len(tok)
    return cams, np.asarray(feats, np.float32).reshape(-1, 3), np.asarray(cols), refs


# ------------------------------------------------------------ reader fixtures
def base_model():
    """Ids with gaps, out of order; an image without 2D points; a name with a
    space; two cameras of different models."""
    cameras = {
        7: dict(model="OPENCV", width=96, height=64,
                params=np.array([82.0, 79.5, 47.25, 31.5, -0.25, 0.08, 0.01, -0.02])),
        2: dict(model="SIMPLE_RADIAL", width=64, height=48,
                params=np.array([70.0, 32.0, 24.0, -0.1])),
    }
    images = {
        12: dict(q=np.array([0.5, -0.5, 0.5, 0.5]), t=np.array([0.1, -2.0, 3.5]), camera_id=2,
                 name="dir with space/img 12.png", xys=np.array([[1.5, 2.25], [30.0, 40.125]]),
                 point3D_ids=np.array([9, -1], np.int64)),
        3: dict(q=np.array([1.0, 0.0, 0.0, 0.0]), t=np.array([0.0, 0.0, 0.0]), camera_id=7,
                name="a.jpg", xys=np.zeros((0, 2)), point3D_ids=np.zeros(0, np.int64)),
        5: dict(q=np.array([0.9238795325112867, 0.0, 0.3826834323650898, 0.0]),
                t=np.array([-1.25, 1e-3, 7.0]), camera_id=7, name="b.JPG",
                xys=np.array([[0.5, 0.5], [95.5, 63.5], [10.0, 11.0]]),
                point3D_ids=np.array([4, 9, 1000000], np.int64)),
    }
    points = {
        1000000: dict(xyz=np.array([0.25, -1.5, 4.0]), rgb=np.array([1, 2, 3], np.uint8),
                      error=0.75, image_ids=np.array([5], np.uint32),
                      point2D_idxs=np.array([2], np.uint32)),
        4: dict(xyz=np.array([1.0, 2.0, 3.0]), rgb=np.array([255, 0, 128], np.uint8), error=1.5,
                image_ids=np.array([5, 3], np.uint32), point2D_idxs=np.array([0, 0], np.uint32)),
        9: dict(xyz=np.array([-1e-3, 1e3, 0.1]), rgb=np.array([9, 9, 9], np.uint8), error=0.0,
                image_ids=np.array([12, 5], np.uint32), point2D_idxs=np.array([0, 1], np.uint32)),
        11: dict(xyz=np.array([0.0, 0.0, 1.0]), rgb=np.array([0, 0, 0], np.uint8), error=2.0,
                 image_ids=np.zeros(0, np.uint32), point2D_idxs=np.zeros(0, np.uint32)),
    }
    return dict(cameras=cameras, images=images, points3D=points)


def _write_files(path, files):
    os.makedirs(path, exist_ok=True)
    for name, data in files.items():
        with open(os.path.join(path, name), "wb" if isinstance(data, bytes) else "w") as f:
            f.write(data)


def _text_files(model, tmp):
    write_text(tmp, model)
    return {n: open(os.path.join(tmp, n)).read()
            for n in ("cameras.txt", "images.txt", "points3D.txt")}


def write_fixtures(root):
    """Writes every reader fixture under `root` -> [(directory, reads fine,
    text the error has to hold or None)]."""
    import copy
    out = []
    model = base_model()
    write_text(os.path.join(root, "text"), model)
    out.append((os.path.join(root, "text"), True, None))
    write_binary(os.path.join(root, "binary"), model)
    out.append((os.path.join(root, "binary"), True, None))
    files, bounds = binary_sections(model)
    good_bin = dict(zip(BIN_NAMES, files))
    good_txt = _text_files(model, os.path.join(root, "_scratch"))

    def add(name, changed, needle):
        path = os.path.join(root, name)
        base = good_bin if next(iter(changed)).endswith(".bin") else good_txt
        _write_files(path, dict(base, **changed))
        out.append((path, False, needle))

    # camera models that are not read: named, never a silent pinhole
    for name, k in UNSUPPORTED.items():
        m = copy.deepcopy(model)
        m["cameras"][7] = dict(model=name, width=96, height=64, params=np.arange(k) + 1.0)
        add("unsupported_%s_txt" % name, dict(_text_files(m, os.path.join(root, "_scratch"))),
            name)
        add("unsupported_%s_bin" % name, {"cameras.bin": binary_sections(m)[0][0]}, name)
    add("unknown_model_txt", {"cameras.txt": "1 KANNALA_BRANDT 4 4 1 2 3 4\n"}, "KANNALA_BRANDT")
    add("unknown_model_bin", {"cameras.bin": struct.pack("<QIiQQ", 1, 1, 99, 4, 4)}, "99")
    # binary files cut at every record boundary and in the middle of every record
    for name, data, b in zip(BIN_NAMES, files, bounds):
        cuts = {0, 4} | set(int(x) for x in b[:-1]) \
            | set(int((lo + hi) // 2) for lo, hi in zip(b[:-1], b[1:]))
        for cut in sorted(cuts):
            add("cut_%s_%d" % (name.replace(".", "_"), cut), {name: data[:cut]}, name)
        add("tail_%s" % name.replace(".", "_"), {name: data + b"\0"}, name)
    # counts that overrun the file
    add("overrun_cameras", {"cameras.bin": struct.pack("<Q", 1 << 60) + files[0][8:]},
        "cameras.bin")
    add("overrun_images", {"images.bin": struct.pack("<Q", 1 << 59) + files[1][8:]},
        "images.bin")
    add("overrun_points", {"points3D.bin": struct.pack("<Q", 1 << 58) + files[2][8:]},
        "points3D.bin")
    one = struct.pack("<QI4d3dI", 1, 3, 1, 0, 0, 0, 0, 0, 0, 7)
    add("overrun_points2d", {"images.bin": one + b"a.jpg\0" + struct.pack("<Q", 1 << 61)},
        "images.bin")
    add("unterminated_name", {"images.bin": one + b"a.jpg" + b"\x01" * 16}, "not terminated")
    add("overrun_track", {"points3D.bin": struct.pack("<QQ3d3BdQ", 1, 4, 1, 2, 3, 1, 2, 3, 0.5,
                                                      1 << 62)}, "points3D.bin")
    # ids across the files
    m = copy.deepcopy(model)
    m["images"][5]["camera_id"] = 42
    add("no_such_camera_txt", dict(_text_files(m, os.path.join(root, "_scratch"))), "42")
    add("no_such_camera_bin", {"images.bin": binary_sections(m)[0][1]}, "42")
    add("duplicate_camera", {"cameras.txt": good_txt["cameras.txt"]
                             + "7 PINHOLE 4 4 1 1 2 2\n"}, "cameras.txt")
    # text files cut in the middle of a record
    lines = good_txt["cameras.txt"].splitlines()
    add("cut_cameras_txt", {"cameras.txt": "\n".join(lines[:-1] + [lines[-1].rsplit(" ", 2)[0]])},
        "cameras.txt")
    lines = good_txt["images.txt"].splitlines()
    add("cut_images_txt_no_points_line", {"images.txt": "\n".join(lines[:-1]) + "\n"},
        "images.txt")
    add("cut_images_txt_first_line", {"images.txt": "\n".join(
        lines[:-2] + [" ".join(lines[-2].split(" ")[:6])])}, "images.txt")
    add("cut_images_txt_triple", {"images.txt": "\n".join(
        lines[:-1] + [lines[-1].rsplit(" ", 1)[0]]) + "\n"}, "images.txt")
    lines = good_txt["points3D.txt"].splitlines()
    add("cut_points_txt", {"points3D.txt": "\n".join(lines[:-1] + [" ".join(
        lines[-1].split(" ")[:5])])}, "points3D.txt")
    add("cut_points_txt_track", {"points3D.txt": "\n".join(
        lines[:-2] + [lines[-2].rsplit(" ", 1)[0]] + lines[-1:]) + "\n"}, "points3D.txt")
    add("not_a_number_txt", {"points3D.txt": "1 0.5 x 3 1 2 3 0.5\n"}, "points3D.txt")
    add("missing_file", {"images.txt": good_txt["images.txt"]}, None)
    os.remove(os.path.join(root, "missing_file", "points3D.txt"))
    return out
