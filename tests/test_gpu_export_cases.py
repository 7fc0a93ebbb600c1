"""smvs_points_generate, smvs_mesh_generate, smvs_simplified_generate and
smvs_simplify_triangulate on the runs of tests/export_cases.py, where every
rule of DESIGN.md section 9 decides (test_export_cases_cpu.py holds the floors
and the variants each run catches), against the serial restatements
tests/points_reference.cc, mesh_reference.cc and simplify_reference.cc.

Everything is compared with array_equal -- positions, colours, confidences,
values, looked-up normals, faces, the vertex order, iterations, triangle
triples, num_zero_depths -- except the normals of recalc_normals (M3-M5), whose
acosf differs between device and host.  Their zero normals coincide exactly;
the others stay within the project's 1e-6 wherever the
restatement itself is that close to M3-M5 evaluated in float64 on the
(bit-equal) positions and faces.  Where it is not -- a vertex on nearly
opposite faces has a short sum -- the device may deviate from float64 by at
most 4 times what the restatement does on that run: two float acosf a few ulps
apart each.  Both deviations are printed (EXPORT_NORMALS)."""
import numpy as np
import pytest

import export_cases as ec  # tests/export_cases.py

pytestmark = pytest.mark.gpu

NORMAL_TOL = 1e-6
NORMAL_FACTOR = 4.0
POINT_KEYS = ("xyz", "normals", "rgb", "confidence", "value")
MESH_KEYS = ("xyz", "rgb", "confidence", "faces")
PLAIN_SIMPLIFY_RUNS = tuple(r for r in ec.SIMPLIFY_RUNS if not r.aabb)


@pytest.fixture(scope="module")
def hip():
    import smvs_amd
    if smvs_amd.device_count() < 1:
        pytest.fail("no HIP device")
    return smvs_amd


def _first_difference(key, got, want):
    """None, or where two arrays first differ."""
    if got.shape != want.shape:
        return "%s: device %s restatement %s" % (key, got.shape, want.shape)
    bad = np.argwhere(~((got == want) | ((got != got) & (want != want))))
    if len(bad) == 0:
        return None
    at = tuple(bad[0])
    return "%s: first of %d differences at %s: device %r restatement %r" % (
        key, len(bad), at, got[at], want[at])


def _assert_equal(got, want, keys, label):
    for k in keys:
        message = _first_difference(k, got[k], want[k])
        assert message is None, label + " " + message


def _assert_normals(got, want, label):
    """The rule of the module's docstring on a mesh dict pair whose positions
    and faces are already known to be equal."""
    g, w = got["normals"].astype(np.float64), want["normals"].astype(np.float64)
    assert np.array_equal(np.all(g == 0, axis=1), np.all(w == 0, axis=1)), label
    diff = float(np.abs(g - w).max()) if len(g) else 0.0
    dev_ref = ec.normal_deviation(want)
    dev_gpu = ec.normal_deviation(got)
    print("EXPORT_NORMALS %-30s vertices %d faces %d device-restatement %.3g "
          "restatement-f64 %.3g device-f64 %.3g" % (label, len(g), len(got["faces"]), diff,
                                                    dev_ref, dev_gpu))
    if dev_ref <= NORMAL_TOL:
        assert diff <= NORMAL_TOL, label
    else:
        assert dev_gpu <= NORMAL_FACTOR * dev_ref, label


def _views(run):
    c = ec.get(run.case)
    return c.cams, c.depths, c.normals, c.images


# ------------------------------------------------------------ regular grid
@pytest.mark.parametrize("run", ec.REGULAR_RUNS, ids=[r.id for r in ec.REGULAR_RUNS])
def test_points(hip, oracle, run):
    box = ec.box(run)
    got = hip.generate_points(*_views(run), cut=run.cut, aabb=box, faces=box is None,
                              dd_factor=run.dd_factor, cut_maps=True)
    want = ec.restated_points(run, oracle=oracle)
    if run.cut:
        for a, b in zip(got["cut_depth"], ec.maps(run.case, oracle)[0]):
            assert np.array_equal(a, b)
    assert len(want["xyz"]) > 0
    _assert_equal(got, want, POINT_KEYS + (("faces",) if box is None else ()), run.id)


@pytest.mark.parametrize("run", ec.REGULAR_RUNS, ids=[r.id for r in ec.REGULAR_RUNS])
def test_mesh(hip, oracle, run):
    got = hip.generate_mesh(*_views(run), cut=run.cut, aabb=ec.box(run), dd_factor=run.dd_factor)
    want = ec.restated_mesh(run, oracle=oracle)
    assert len(want["faces"]) > 0 and "value" not in got
    _assert_equal(got, want, MESH_KEYS, run.id)
    _assert_normals(got, want, run.id)


def test_a_one_column_view_contributes_nothing(hip):
    """A 1 x N view has no block: the entries accept it and the call equals the
    one without it (face-id offsets included); so does a view without depth."""
    for name, drop in (("mixed_sizes", ec.ONE_COLUMN_VIEW), ("all_holes_view", 1)):
        c = ec.get(name)
        assert min(c.depths[drop].shape) == 1 or not c.depths[drop].any()
        parts = (c.cams, c.depths, c.normals, c.images)
        rest = [[x for i, x in enumerate(p) if i != drop] for p in parts]
        with_it = hip.generate_points(*parts, cut=False, faces=True)
        without = hip.generate_points(*rest, cut=False, faces=True)
        _assert_equal(with_it, without, POINT_KEYS + ("faces",), name)
        with_it = hip.generate_mesh(*parts, cut=False)
        without = hip.generate_mesh(*rest, cut=False)
        _assert_equal(with_it, without, MESH_KEYS + ("normals",), name)


# --------------------------------------------------------------- simplified
@pytest.mark.parametrize("run", PLAIN_SIMPLIFY_RUNS, ids=[r.id for r in PLAIN_SIMPLIFY_RUNS])
def test_triangulation(hip, run):
    """S1-S8 insertion by insertion, every view of the run."""
    for view, dm in enumerate(ec.get(run.case).depths):
        got = hip.simplify_triangulate(dm, max_vertices=run.max_vertices,
                                       max_error=run.max_error)
        want = ec.restated_triangulation(run, view)
        label = "%s view %d (%d x %d)" % (run.id, view, dm.shape[1], dm.shape[0])
        print("EXPORT_TRI %s iterations %d/%d vertices %d triangles %d" % (
            label, got["iterations"], want["iterations"], len(got["vertices"]),
            len(got["triangles"])))
        assert got["iterations"] == want["iterations"], label
        n = min(len(got["vertices"]), len(want["vertices"]))
        differ = np.nonzero((got["vertices"][:n] != want["vertices"][:n]).any(axis=1))[0]
        assert len(differ) == 0, "%s: first differing insertion: vertex %d" % (label, differ[0])
        _assert_equal(got, want, ("vertices", "triangles", "num_zero_depths"), label)


@pytest.mark.parametrize("mesh", [False, True], ids=["points", "mesh"])
@pytest.mark.parametrize("run", ec.SIMPLIFY_RUNS, ids=[r.id for r in ec.SIMPLIFY_RUNS])
def test_simplified(hip, run, mesh):
    box = ec.box(run)
    got = hip.generate_simplified(*_views(run), mesh=mesh, cut=False, aabb=box,
                                  max_vertices=run.max_vertices, max_error=run.max_error)
    want = ec.restated_simplified(run, mesh)
    keys = ["xyz", "rgb", "confidence"]
    if mesh or box is None:
        keys.append("faces")
    else:
        assert "faces" not in got
    if mesh:
        assert "value" not in got
    else:
        keys += ["value", "normals"]
    _assert_equal(got, want, keys, "%s mesh %d" % (run.id, mesh))
    if mesh:
        _assert_normals(got, want, "%s" % run.id)


def test_simplified_refuses_the_one_column_view(hip):
    from smvs_amd._capi import SmvsError
    c = ec.get("mixed_sizes")
    with pytest.raises(SmvsError):
        hip.generate_simplified(c.cams, c.depths, c.normals, c.images, cut=False)
    with pytest.raises(SmvsError):
        hip.simplify_triangulate(c.depths[ec.ONE_COLUMN_VIEW])
