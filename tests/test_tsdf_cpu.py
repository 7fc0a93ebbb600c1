"""The volumetric fusion's definition (tests/tsdf_ref.py, the numpy restatement
of include/smvs_hip.h's smvs_tsdf_fuse) on exact, noise-free depth maps of the
synthetic sphere: the mesh is a consistently oriented manifold piece that lies
on the sphere.  And, where the library loads, every refusal of the entry
(argument errors are status codes before any device call).  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import mesh_ref  # tests/mesh_ref.py
import tsdf_ref  # tests/tsdf_ref.py

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

W, H, VIEWS = 128, 96, 6
ORIGIN = (-1.15, -1.15, 2.85)
VOXEL = 0.05
DIMS = (46, 46, 28)
TRUNC = 3 * VOXEL


@pytest.fixture(scope="module")
def sphere():
    from smvs_amd import synth
    inputs = synth.pipeline_inputs("sphere", W, H, VIEWS - 1, flen=1.2)
    cams = inputs["cams"]
    assert len(cams) == VIEWS
    depths, normals = synth.depth_and_normal_maps(inputs["scene"], cams)
    images = inputs["images"]
    mesh = tsdf_ref.fuse(cams, depths, images, ORIGIN, VOXEL, DIMS)
    for a in mesh.values():
        a.setflags(write=False)
    return inputs["scene"], cams, depths, normals, images, mesh


def test_mesh_is_well_formed(sphere):
    mesh = sphere[5]
    faces = mesh["faces"].astype(np.int64)
    assert len(faces) > 0 and len(mesh["xyz"]) > 0
    assert faces.max() < len(mesh["xyz"])
    assert np.all(np.isfinite(mesh["xyz"]))
    # every undirected edge belongs to at most two faces
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    e.sort(axis=1)
    _, counts = np.unique(e, axis=0, return_counts=True)
    assert counts.max() <= 2
    # a face has three different corners
    assert np.all(faces[:, 0] != faces[:, 1]) and np.all(faces[:, 1] != faces[:, 2]) \
        and np.all(faces[:, 0] != faces[:, 2])


def test_orientation(sphere):
    scene, mesh = sphere[0], sphere[5]
    xyz = mesh["xyz"].astype(np.float64)
    nrm = mesh["normals"].astype(np.float64)
    has = np.any(nrm != 0, axis=1)
    assert has.sum() > 0.9 * len(xyz)
    # normals point out of the sphere
    assert np.all(np.sum(nrm[has] * (xyz[has] - scene.c), axis=1) > 0)
    # the winding of every face agrees with its vertices' normals
    f = mesh["faces"].astype(np.int64)
    fn = np.cross(xyz[f[:, 1]] - xyz[f[:, 0]], xyz[f[:, 2]] - xyz[f[:, 0]])
    for k in range(3):
        use = has[f[:, k]]
        assert np.all(np.sum(fn[use] * nrm[f[use, k]], axis=1) > 0), k


def test_vertices_lie_on_the_sphere(sphere, oracle):
    """An active cell has an inside corner; that corner has, in some view,
    -trunc <= sdf < 0 against an exact depth; the distance along z to a surface
    point bounds the distance to the surface; the vertex lies in the corner's
    cell: trunc + one voxel diagonal."""
    scene, cams, depths, normals, images, mesh = sphere
    xyz = mesh["xyz"].astype(np.float64)
    dist = np.abs(np.linalg.norm(xyz - scene.c, axis=1) - scene.r)
    dms, wn = oracle.cut_depth_maps(cams, depths, normals)
    per_view = mesh_ref.mesh(cams, dms, wn, images)
    text = ("# tests/test_tsdf_cpu.py: tests/tsdf_ref.py on the synthetic sphere, %d exact depth maps\n"
            "# of %d x %d, box %s, voxel %.3g, dims %s, trunc 3 voxels.  Reported, not asserted.\n"
            "distance of the vertices to the true sphere, in voxels: median %.4f  max %.4f\n"
            "vertices %d  faces %d  (per-view triangulations merged, mesh_ref on the cut maps: "
            "%d vertices, %d faces)\n"
            % (VIEWS, W, H, ORIGIN, VOXEL, DIMS, np.median(dist) / VOXEL, dist.max() / VOXEL,
               len(xyz), len(mesh["faces"]), len(per_view["xyz"]), len(per_view["faces"])))
    print(text)
    try:
        with open(os.path.join(ROOT, "profiles", "tsdf_synth_accuracy.txt"), "w") as f:
            f.write(text)
    except OSError:
        pass    # a read-only tree: the figures are printed above
    assert dist.max() <= TRUNC + np.sqrt(3.0) * VOXEL


def test_field_signs_and_unknowns(sphere):
    """The field itself: negative just inside the sphere's visible front,
    positive in front of it, unknown far behind it."""
    scene, mesh = sphere[0], sphere[5]
    F = mesh["tsdf"]
    i, j = DIMS[0] // 2, DIMS[1] // 2
    z = ORIGIN[2] + (np.arange(DIMS[2]) + 0.5) * VOXEL
    column = F[:, j, i]
    front = scene.c[2] - scene.r
    assert np.all(column[z < front - VOXEL] > 0)
    inside = (z > front + VOXEL) & (z < front + TRUNC - VOXEL)
    assert inside.any() and np.all(column[inside] < 0)
    assert np.all(np.isnan(column[z > front + TRUNC + 2 * VOXEL]))
    assert np.all(mesh["weight"][np.isnan(F)] == 0)


# ------------------------------------------------------------------ refusals
@pytest.fixture(scope="module")
def lib():
    from smvs_amd import build as hip_build, _capi
    hip_build.build()
    return _capi.load()


def _call(lib, n=2, normals=True, depth=True, image=True, channels=3, **changes):
    from smvs_amd import synth, _capi
    from smvs_amd.device import _tsdf_views
    main, subs = synth.ring_cameras(16, 12, 1)
    cams = [main] + subs
    depths = [np.full((12, 16), 4.0, np.float32) for _ in cams]
    nm = [np.zeros((12, 16, 3), np.float32) for _ in cams] if normals else None
    images = [np.zeros((12, 16, 3), np.uint8) for _ in cams]
    arr, _keep = _tsdf_views(cams, depths, nm, images)
    if not depth:
        arr[1].depth = None
    if not image:
        arr[1].image = None
    arr[1].channels = channels
    opt = _capi.TsdfOptions()
    values = dict(cut_surfaces=1, origin=(-1.0, -1.0, 3.0), voxel_size=0.25, dims=(8, 8, 8),
                  trunc=0.0, min_weight=0)
    values.update(changes)
    opt.cut_surfaces = values["cut_surfaces"]
    opt.voxel_size = values["voxel_size"]
    opt.trunc = values["trunc"]
    opt.min_weight = values["min_weight"]
    for k in range(3):
        opt.origin[k] = values["origin"][k]
        opt.dims[k] = values["dims"][k]
    handle = C.c_void_p(1)
    nv, nf = C.c_int64(-7), C.c_int64(-7)
    rc = lib.smvs_tsdf_fuse(0, arr if n > 0 else None, n, C.byref(opt), None, None,
                            C.byref(handle), C.byref(nv), C.byref(nf))
    return rc, handle.value


REFUSED = [
    dict(n=0), dict(n=-1),
    dict(voxel_size=0.0), dict(voxel_size=-0.1), dict(voxel_size=float("nan")),
    dict(voxel_size=float("inf")),
    dict(dims=(1, 8, 8)), dict(dims=(8, 8, 1)), dict(dims=(8, 1025, 8)), dict(dims=(8, 8, 0)),
    dict(dims=(1024, 1024, 1024)), dict(dims=(1024, 1024, 129)),
    dict(origin=(float("nan"), 0.0, 0.0)), dict(origin=(0.0, 0.0, float("inf"))),
    dict(trunc=float("nan")),
    dict(normals=False, cut_surfaces=1),
    dict(depth=False), dict(image=False), dict(channels=0), dict(channels=5),
]


@pytest.mark.parametrize("case", REFUSED, ids=lambda c: ",".join("%s=%s" % kv for kv in c.items()))
def test_refusals_are_status_codes(lib, case):
    """Before any device call: the same status with or without a device."""
    lib.smvs_last_error.restype = C.c_char_p
    rc, handle = _call(lib, **case)
    assert rc == -1, lib.smvs_last_error()
    assert handle is None


def test_other_refusals(lib):
    from smvs_amd import synth
    from smvs_amd.device import _tsdf_views
    main, subs = synth.ring_cameras(16, 12, 1)
    depths = [np.full((12, 16), 4.0, np.float32)] * 2
    arr, _keep = _tsdf_views([main] + subs, depths, None, None)
    lo = (C.c_float * 3)()
    hi = (C.c_float * 3)()
    # no options, no handle pointer
    handle = C.c_void_p(1)
    assert lib.smvs_tsdf_fuse(0, arr, 2, None, None, None, C.byref(handle), None, None) == -1
    assert lib.smvs_tsdf_fuse(0, arr, 2, None, None, None, None, None, None) == -1
    # the bounds: no views, no outputs, the cut without normals
    assert lib.smvs_tsdf_bounds(0, None, 0, 0, lo, hi) == -1
    assert lib.smvs_tsdf_bounds(0, arr, 2, 0, None, hi) == -1
    assert lib.smvs_tsdf_bounds(0, arr, 2, 1, lo, hi) == -1
    if lib.smvs_device_count() < 1:
        # accepted arguments reach the device, and without one that is an error
        # of its own, not an argument error
        assert _call(lib, normals=False, cut_surfaces=0)[0] == -2
        assert lib.smvs_tsdf_bounds(0, arr, 2, 0, lo, hi) == -2
