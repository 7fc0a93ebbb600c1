"""What the scene entry of the fused mesh (smvs_host_generate_fused* in
csrc/host/host_capi.h, host.generate_fused in front of it) refuses, pinned:
status and exact smvs_host_last_error() text of calls that each end before the
first device call, recorded in tests/golden/fused_entry_refusals.json.

The scene is written without a device: two plane views with their rendered
depth and normal maps as smvs-B0 / smvs-B0N.  The three paths behind the
entries (unbatched, batch_views, sparse_batch_views) check in different orders
and not the same set; cases that violate two checks at once pin the order, and
one case pins a call that succeeds: without a usable view the unbatched path
returns an empty mesh before it looks at the resolution, the batched path
refuses the resolution first.  All of it is the contract.

`python tests/test_fused_entry_refusals_cpu.py --record` rewrites the JSON from
the library as built; it was recorded before the three paths were merged."""
import ctypes as C
import json
import os
import sys
import tempfile

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "fused_entry_refusals.json")

_i32p = C.POINTER(C.c_int32)
EMPTY_AABB = ((0.5, -1.0, 2.0), (-0.5, 1.0, 4.0))     # min above max on x
ENTRIES = ("_fused", "_fused_sparse", "_fused_sparse_cull", "_fused_clean", "_fused_batched",
           "_fused_sparse_batched")


def write_scene(d):
    from smvs_amd import mve_scene, synth
    inputs = synth.pipeline_inputs("plane", 48, 32, 2, n_features=20)
    mve_scene.write_scene(d, inputs)
    depths, normals = synth.depth_and_normal_maps(inputs["scene"], inputs["cams"])
    for i, (depth, normal) in enumerate(zip(depths, normals)):
        view = os.path.join(d, "views", "view_%04d.mve" % i)
        mve_scene.save_mvei(os.path.join(view, "smvs-B0.mvei"), depth)
        mve_scene.save_mvei(os.path.join(view, "smvs-B0N.mvei"), normal)
    return d


def front(scene_dir, input_scale=0, **kw):
    """host.generate_fused -> (status, text, result)"""
    from smvs_amd import host
    from smvs_amd._capi import SmvsError
    try:
        out = host.generate_fused(scene_dir, cut=False, input_scale=input_scale, **kw)
    except SmvsError as e:
        return e.status, host.load().smvs_host_last_error().decode(), None
    os.remove(out[0])
    return 0, "", [os.path.basename(out[0])] + [int(x) for x in out[1:]]


def record_of(entry, resolution=64, max_bricks=0, cull=0, sparse=0, batch_views=0,
              sparse_batch_views=0):
    """the settings record of smvs_host_generate<entry>, cut to its members"""
    from smvs_amd import host
    cls = dict(_fused=host.FusedSettings, _fused_sparse=host.FusedSparseSettings,
               _fused_sparse_cull=host.FusedSparseCullSettings,
               _fused_clean=host.FusedCleanSettings, _fused_batched=host.FusedBatchedSettings,
               _fused_sparse_batched=host.FusedSparseBatchedSettings)[entry]
    widest = (0.0, resolution, 0.0, 0, max_bricks, cull, sparse, 0.0, 0.0, 1000, 0, 0,
              batch_views, sparse_batch_views)
    return cls(*widest[:len(cls._fields_)])


def direct(scene_dir, entry, null_record=False, **kw):
    """smvs_host_generate<entry> through ctypes -> (status, text, result)"""
    from smvs_amd import _capi, host
    lib = host.load()
    st = host.PointCloudSettings()
    st.image_embedding = b"undistorted"
    fs = record_of(entry, **kw)
    path = C.create_string_buffer(4096)
    nv, nf = C.c_int64(0), C.c_int64(0)
    args = [scene_dir.encode(), C.byref(st), None if null_record else C.byref(fs), None,
            C.c_int(0), path, C.c_int(len(path)), C.byref(nv), C.byref(nf)]
    if entry in ENTRIES[3:]:
        stats = _capi.MeshCleanStats()
        args.append(C.byref(stats))
    status = int(getattr(lib, "smvs_host_generate" + entry)(*args))
    return status, lib.smvs_host_last_error().decode() if status else "", None


def _build_cases():
    c = {}
    # ---- through host.generate_fused
    paths = {"dense": dict(), "sparse": dict(sparse=True), "batched": dict(batch_views=2),
             "sparse_batched": dict(sparse=True, sparse_batch_views=2)}
    for name, kw in paths.items():
        c["front/resolution4/" + name] = lambda d, kw=kw: front(d, resolution=4, **kw)
    for name in ("sparse", "sparse_batched"):
        c["front/resolution5000/" + name] = \
            lambda d, kw=paths[name]: front(d, resolution=5000, **kw)
    c["front/sparse+batch_views"] = lambda d: front(d, resolution=64, sparse=True, batch_views=2)
    c["front/batch_views-1"] = lambda d: front(d, resolution=64, batch_views=-1)
    c["front/sparse_batch_views-1"] = \
        lambda d: front(d, resolution=64, sparse=True, sparse_batch_views=-1)
    c["front/both_batch_options"] = \
        lambda d: front(d, resolution=64, sparse=True, batch_views=2, sparse_batch_views=2)
    for name in ("dense", "batched", "sparse_batched"):
        c["front/empty_aabb/" + name] = \
            lambda d, kw=paths[name]: front(d, resolution=64, aabb=EMPTY_AABB, **kw)
    # no view has smvs-B3: the unbatched path succeeds, the batched one refuses
    c["front/no_usable_view+resolution4/dense"] = lambda d: front(d, input_scale=3, resolution=4)
    c["front/no_usable_view+resolution4/batched"] = \
        lambda d: front(d, input_scale=3, resolution=4, batch_views=2)
    # ---- through ctypes: what host.generate_fused refuses before the library
    wide = (("_fused_clean", dict()), ("_fused_batched", dict()),
            ("_fused_batched", dict(batch_views=2)), ("_fused_sparse_batched", dict()),
            ("_fused_sparse_batched", dict(batch_views=2)))
    for entry, kw in wide:
        tag = "direct%s%s/" % (entry, "/batch_views2" if kw else "")
        c[tag + "max_bricks_dense"] = \
            lambda d, e=entry, kw=kw: direct(d, e, max_bricks=7, **kw)
        c[tag + "cull_dense"] = lambda d, e=entry, kw=kw: direct(d, e, cull=1, **kw)
        c[tag + "max_bricks+cull_dense"] = \
            lambda d, e=entry, kw=kw: direct(d, e, max_bricks=7, cull=1, **kw)
    c["direct_fused_sparse_batched/sparse_batch_views_dense"] = \
        lambda d: direct(d, "_fused_sparse_batched", sparse_batch_views=2)
    for entry in ENTRIES:
        c["direct%s/null_record" % entry] = lambda d, e=entry: direct(d, e, null_record=True)
    return c


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


CASE_IDS = sorted(_golden()) if os.path.exists(GOLDEN) else []


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return write_scene(str(tmp_path_factory.mktemp("refusals")))


def test_table_and_golden_hold_the_same_cases():
    assert sorted(_build_cases()) == CASE_IDS
    assert len(CASE_IDS) == 37


@pytest.mark.parametrize("case", CASE_IDS)
def test_refusal(scene_dir, case):
    want = _golden()[case]
    status, text, result = _build_cases()[case](scene_dir)
    assert status == want["status"], (case, status, text)
    assert text == want["error"], (case, text)
    assert result == want["result"], (case, result)


def test_the_recorded_orders_and_asymmetries():
    """Spot checks of what the JSON records, so that a re-recording cannot quietly
    change the contract."""
    g = _golden()
    refused = [k for k in g if g[k]["status"] != 0]
    assert len(refused) == len(g) - 1 and all(g[k]["status"] == -1 for k in refused)
    assert g["front/no_usable_view+resolution4/dense"] \
        == dict(status=0, error="", result=["smvs-fused-B3.ply", 0, 0])
    at_least = "generate_fused: resolution must be at least 8"
    assert g["front/no_usable_view+resolution4/batched"]["error"] == at_least
    for name in ("dense", "sparse", "batched", "sparse_batched"):
        assert g["front/resolution4/" + name]["error"] == at_least
    for name in ("sparse", "sparse_batched"):
        assert g["front/resolution5000/" + name]["error"] \
            == "generate_fused: resolution must be at most 4096"
    dense_volume = "generate_fused: batch_views belongs to the dense volume"
    assert g["front/sparse+batch_views"]["error"] == dense_volume
    assert g["front/both_batch_options"]["error"] == dense_volume
    assert g["front/batch_views-1"]["error"] == "generate_fused: batch_views must not be negative"
    for name in ("dense", "batched", "sparse_batched"):
        assert g["front/empty_aabb/" + name]["error"] == "generate_fused: the box is empty"
    for k in g:
        if k.endswith("/max_bricks_dense") or k.endswith("/max_bricks+cull_dense"):
            assert g[k]["error"] == "generate_fused: max_bricks belongs to sparse", k
        if k.endswith("/cull_dense"):
            assert g[k]["error"].endswith(" belongs to sparse"), k
    for entry in ENTRIES:
        assert g["direct%s/null_record" % entry]["error"] \
            == "smvs_host_generate%s: bad argument" % entry


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit("usage: %s --record" % sys.argv[0])
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    out = {}
    with tempfile.TemporaryDirectory() as d:
        write_scene(d)
        for name, call in sorted(_build_cases().items()):
            status, text, result = call(d)
            out[name] = dict(status=status, error=text, result=result)
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded", len(out), "cases in", GOLDEN)
