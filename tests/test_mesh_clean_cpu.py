"""The mesh clean's restatement (tests/mesh_clean_ref.py) against answers
written by hand and, where scipy imports, against scipy's components; the tally
of the cases the GPU tests run (tests/mesh_clean_cases.py), which keeps a GPU
pass from being vacuous; and what smvs_mesh_clean refuses before any device
call.  No GPU needed.

The tally is a condition on the inputs, not a measurement of the device.
`python tests/test_mesh_clean_cpu.py` prints it and writes profiles/
mesh_clean_cases_tally.txt, which test_tally compares with the builders."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_clean_cases as cases  # noqa: E402  tests/mesh_clean_cases.py
import mesh_clean_ref as ref  # noqa: E402  tests/mesh_clean_ref.py

NONE = 0xFFFFFFFF


def test_small_mesh_by_hand():
    mesh = cases.small_mesh()
    out = ref.clean(mesh, threshold=0.1, component_size=4)
    assert out["component"].tolist() == [0, 0, 0, 0, 4, 5, 6, 7, NONE, 9]
    assert out["component_size"].tolist() == [4, 4, 4, 4, 1, 1, 1, 1, 0, 1]
    assert out["new_id"].tolist() == [0, 1, 2, 3, -1, -1, -1, -1, -1, -1]
    assert out["faces"].tolist() == [[0, 1, 2], [2, 1, 3]]
    for k in ("xyz", "normals", "rgb", "confidence", "cells"):
        assert np.array_equal(out[k], mesh[k][:4]), k
    assert out["stats"] == {"cut_value": float(np.float32(0.1)), "n_cut": 1, "n_components": 6,
                            "n_small_components": 5, "n_small_vertices": 5,
                            "n_unreferenced": 5, "largest_component": 4}
    # component_size 1 makes nothing small; the unreferenced go or stay
    out = ref.clean(mesh, threshold=0.1, component_size=1)
    assert out["new_id"].tolist() == [0, 1, 2, 3, -1, -1, -1, -1, -1, -1]
    assert out["stats"]["n_small_components"] == 0 and out["stats"]["n_small_vertices"] == 0
    out = ref.clean(mesh, threshold=0.1, component_size=1, keep_unreferenced=True)
    assert out["new_id"].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, -1, 8]
    assert out["faces"].tolist() == [[0, 1, 2], [2, 1, 3]]
    assert np.array_equal(out["confidence"], np.delete(mesh["confidence"], 8))
    # kept unreferenced vertices are still small below component_size
    out = ref.clean(mesh, threshold=0.1, component_size=2, keep_unreferenced=True)
    assert out["new_id"].tolist() == [0, 1, 2, 3, -1, -1, -1, -1, -1, -1]
    # no cut: 7-8-9 is a component of 3
    out = ref.clean(mesh, component_size=3)
    assert out["stats"]["cut_value"] == -np.inf and out["stats"]["n_cut"] == 0
    assert out["new_id"].tolist() == [0, 1, 2, 3, -1, -1, -1, 4, 5, 6]
    assert out["faces"].tolist() == [[0, 1, 2], [2, 1, 3], [4, 5, 6]]
    assert out["component"].tolist() == [0, 0, 0, 0, 4, 5, 6, 7, 7, 7]


def test_cut_value_by_hand():
    conf = np.float32([0.5, np.nan, -0.0, 0.0, 0.25, 0.25, -1.0, 0.25])
    # key order: -1, -0.0, 0.0, 0.25 x 3, 0.5, NaN
    want = [-1.0, -0.0, 0.0, 0.25, 0.25, 0.25, 0.5, np.nan]
    for k, w in enumerate(want):
        p = np.float32(100.0 * k / 7) if k else np.float32(1e-3)   # (0 is "off")
        while int(float(p) * 7.0 / 100.0) < k:
            p = np.nextafter(p, np.float32(200))
        t = ref.cut_value(conf, 0.0, p)
        assert np.float32(t).view(np.uint32) == np.float32(w).view(np.uint32), (k, t, w)
    assert np.isnan(ref.cut_value(conf, 0.0, 100.0))
    assert ref.cut_value(conf, 0.0, 0.0) == -np.inf and ref.cut_value(conf, -1.0, 0.0) == -np.inf
    assert ref.cut_value(conf, 0.3, 0.0) == np.float32(0.3)
    assert ref.cut_value(conf[:0], 0.0, 10.0) == -np.inf
    with pytest.raises(ValueError):
        ref.cut_value(conf, 0.3, 10.0)
    mesh = cases.make_mesh(8, [[0, 1, 2]], 3, conf)
    # t = -0.0: 0.0 < -0.0 is false, only -1 is cut; a NaN t cuts nothing
    out = ref.clean(mesh, percentile=15.0, component_size=1,   # k = 1
                    keep_unreferenced=True)
    assert out["new_id"].tolist() == [0, 1, 2, 3, 4, 5, -1, 6]
    out = ref.clean(mesh, percentile=100.0, component_size=1, keep_unreferenced=True)
    assert out["stats"]["n_cut"] == 0 and np.isnan(out["stats"]["cut_value"])
    # a NaN confidence is never cut
    out = ref.clean(mesh, threshold=10.0, component_size=1, keep_unreferenced=True)
    assert out["new_id"].tolist() == [-1, 0, -1, -1, -1, -1, -1, -1]


@pytest.mark.parametrize("name", cases.case_names())
def test_components_against_scipy(name):
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    from scipy.sparse import coo_matrix
    mesh, _opts, out = cases.case(name)
    comp = out["component"]
    n = comp.size
    uncut = comp != ref.NO_COMPONENT
    f = mesh["faces"].astype(np.int64)
    ok = uncut[f].all(1) & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2]) \
        if f.size else np.zeros(0, bool)
    f = f[ok]
    a = np.concatenate([f[:, 0], f[:, 1]])
    b = np.concatenate([f[:, 1], f[:, 2]])
    _, lab = csgraph.connected_components(coo_matrix((np.ones(a.size), (a, b)), shape=(n, n)),
                                          directed=False)
    # scipy's labels -> the smallest id of each component
    low = np.full(n, n, np.int64)
    np.minimum.at(low, lab, np.arange(n))
    assert np.array_equal(comp[uncut], low[lab][uncut])


def test_strip_is_one_component():
    for order in ("permuted", "reversed"):
        _mesh, _opts, out = cases.case("strip-" + order)
        assert (out["component"] == 0).all() and (out["component_size"] == 5000).all()
        assert out["stats"]["n_components"] == 1 and len(out["faces"]) == 4998
        assert np.array_equal(out["new_id"], np.arange(5000))
    _mesh, _opts, out = cases.case("fan")
    assert out["stats"]["n_components"] == 1 and out["stats"]["largest_component"] == 3000


def test_bridge_splits():
    mesh, a, b, j = cases.bridge()
    _mesh, opts, out = cases.case("bridge")
    whole = ref.clean(mesh, component_size=opts["component_size"])
    assert whole["stats"]["n_components"] == 1 and (whole["new_id"] >= 0).all()
    assert out["component"][j] == ref.NO_COMPONENT and out["stats"]["n_cut"] == 1
    assert (out["component"][a] == a.min()).all() and (out["component"][b] == b.min()).all()
    assert (out["new_id"][a] >= 0).all() and (out["new_id"][b] == -1).all()
    assert out["stats"]["n_small_components"] == 1
    assert out["stats"]["n_small_vertices"] == cases.BRIDGE_B
    assert len(out["faces"]) == cases.BRIDGE_A - 2


def test_group_sizes():
    for n in cases.GROUP_N:
        _mesh, sizes = cases.groups(n, 100 + n, False)
        assert sum(sizes) == n and min(sizes) >= 1 and max(sizes) <= 300
        if n >= 63:
            assert tuple(sizes[:len(cases.FIXED_SIZES)]) == cases.FIXED_SIZES
    for dense in (False, True):
        mesh, _sizes = cases.groups(4097, 100 + 4097, dense)
        assert (mesh["faces"].shape[0] > 4097) == dense


def tally_lines():
    lines = []
    for name in cases.case_names():
        t = cases.tally(name)
        lines.append("tally %-24s n %6d m %6d  small_removed %4d kept %4d kept_at_size %d  cut %5d"
                     " faces_cut %5d faces_repeated %5d  -> n %6d m %6d"
                     % (name, t["n"], t["m"], t["small_removed"], t["kept"], t["kept_at_size"],
                        t["cut"], t["faces_cut"], t["faces_repeated"], t["out_n"], t["out_m"]))
    return lines


TALLY_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
                          "mesh_clean_cases_tally.txt")


def test_tally():
    """Every group case but n = 1 (one vertex: nothing to split) removes >= 3
    components as small, keeps >= 3, keeps >= 1 of exactly component_size, cuts
    >= 1 vertex, loses >= 1 face to the cut and >= 1 to a repeated id: the
    builder's fixed groups (mesh_clean_cases.FIXED_SIZES, 63 vertices) see to
    it at the wave-edge sizes too.  The committed tally is the builders'."""
    lines = tally_lines()
    print("\n".join(lines))
    with open(TALLY_FILE) as f:
        assert f.read().splitlines() == lines, \
            "profiles/mesh_clean_cases_tally.txt: `python tests/test_mesh_clean_cpu.py` rewrites it"
    total = dict.fromkeys(("small_removed", "kept", "kept_at_size", "cut", "faces_cut",
                           "faces_repeated"), 0)
    for name in cases.case_names():
        if not name.startswith("groups-"):
            continue
        t = cases.tally(name)
        for k in total:
            total[k] += t[k]
        if t["n"] == 1:
            continue
        assert t["n"] >= 63
        assert t["small_removed"] >= 3 and t["kept"] >= 3 and t["kept_at_size"] >= 1, (name, t)
        assert t["cut"] >= 1 and t["faces_cut"] >= 1 and t["faces_repeated"] >= 1, (name, t)
    assert all(v >= 3 for v in total.values()), total
    # the empty cases are empty the way they say
    assert cases.tally("all-cut")["out_n"] == 0 and cases.tally("all-cut")["cut"] == 257
    assert cases.tally("empty-m0")["out_n"] == 300 and cases.tally("empty-m0-drop")["out_n"] == 0
    assert cases.tally("empty-n0")["n"] == 0
    # the tie cases place k on a run's first, inner and last element
    mesh, _o, _r = cases.case("ties-p10-comp")
    ks = [k for k, _p in cases.tie_percentiles(mesh["confidence"])]
    key = np.sort(ref.float_key(mesh["confidence"]))
    assert len(ks) == 4 and key[ks[0]] == key[ks[1]] == key[ks[2]] and ks[0] < ks[1] < ks[2]
    assert key[ks[0] - 1] != key[ks[0]] and key[ks[2] + 1] != key[ks[2]]


# ------------------------------------------------------------ the C ABI's refusals
def _lib():
    from smvs_amd import _capi
    return _capi, _capi.load()


def call_clean(lib, _capi, mesh, n=None, m=None, missing=(), **opts):
    """smvs_mesh_clean on `mesh` with arguments overridden -> the status"""
    fp, u8p, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
    arrs = {"xyz": (mesh["xyz"], fp), "normals": (mesh["normals"], fp), "rgb": (mesh["rgb"], u8p),
            "confidence": (mesh["confidence"], fp), "faces": (mesh["faces"], u32p)}
    ptr = {k: (None if k in missing else a.ctypes.data_as(t)) for k, (a, t) in arrs.items()}
    opt = _capi.MeshCleanOptions(opts.get("threshold", 0.0), opts.get("percentile", 0.0),
                                 opts.get("component_size", 1000), 0)
    handle = C.c_void_p()
    rc = lib.smvs_mesh_clean(0, C.c_int64(mesh["confidence"].size if n is None else n),
                             C.c_int64(mesh["faces"].shape[0] if m is None else m), ptr["xyz"],
                             ptr["normals"], ptr["rgb"], ptr["confidence"], None, ptr["faces"],
                             C.byref(opt), None, None, None, None, C.byref(handle), None, None)
    assert rc != 0 and not handle.value
    return rc


REFUSED = [dict(n=-1), dict(m=-1), dict(n=2 ** 31), dict(m=2 ** 31),
           dict(percentile=-0.5), dict(percentile=100.5), dict(percentile=float("nan")),
           dict(percentile=float("inf")), dict(threshold=float("nan")),
           dict(threshold=float("inf")), dict(threshold=0.1, percentile=10.0),
           dict(missing=("xyz",)), dict(missing=("normals",)), dict(missing=("rgb",)),
           dict(missing=("confidence",)), dict(missing=("faces",))]


@pytest.mark.parametrize("how", REFUSED, ids=lambda h: "-".join("%s=%s" % kv for kv in h.items()))
def test_refused_before_any_device_call(how):
    _capi, lib = _lib()
    mesh = cases.small_mesh()
    assert call_clean(lib, _capi, mesh, **how) == -1
    assert b"smvs_mesh_clean" in lib.smvs_last_error()


def test_face_id_refused():
    _capi, lib = _lib()
    mesh = dict(cases.small_mesh())
    for bad in (10, 11, 0xFFFFFFFF):   # 10 == n
        faces = mesh["faces"].copy()
        faces[3, 2] = bad
        assert call_clean(lib, _capi, dict(mesh, faces=faces)) == -1
        assert b"vertex id" in lib.smvs_last_error()
    for name in ("smvs_mesh_clean", "smvs_mesh_clean_handle"):
        assert name in _capi.declared_symbols() and hasattr(lib, name), name
    assert lib.smvs_mesh_clean_handle(0, None, None, None, None, None, None,
                                      C.byref(C.c_void_p()), None, None) == -1


def test_host_entry_refuses_bad_arguments():
    from smvs_amd import host
    lib = host.load()
    st = host._point_cloud_settings("undistorted", 0, False, True, None, True, False, 0)
    fs = host.FusedCleanSettings(0.0, 64, 0.0, 0, 0, 0, 0, 0.0, 10.0, 50, 0)
    path = C.create_string_buffer(64)
    nv, nf = C.c_int64(), C.c_int64()
    for scene, settings, fused in ((None, C.byref(st), C.byref(fs)), (b"/nowhere", None, C.byref(fs)),
                                   (b"/nowhere", C.byref(st), None)):
        assert lib.smvs_host_generate_fused_clean(scene, settings, fused, None, 0, path, 64,
                                                  C.byref(nv), C.byref(nf), None) != 0
        assert lib.smvs_host_last_error() == b"smvs_host_generate_fused_clean: bad argument"
    # a scene that is not there: the scene loader's error, not a crash
    assert lib.smvs_host_generate_fused_clean(b"/nowhere", C.byref(st), C.byref(fs), None, 0, path,
                                              64, C.byref(nv), C.byref(nf), None) != 0
    with pytest.raises(ValueError):
        host.generate_fused("/nowhere", clean=dict(percentil=10))
    with pytest.raises(ValueError):
        host.generate_fused("/nowhere", cull=True, clean=dict(percentile=10))


if __name__ == "__main__":
    with open(TALLY_FILE, "w") as out:
        out.write("\n".join(tally_lines()) + "\n")
    print("\n".join(tally_lines()))
