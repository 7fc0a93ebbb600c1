"""The brick-sparse fusion's definition (tests/tsdf_sparse_ref.py, the comment of
smvs_tsdf_fuse_sparse in include/smvs_hip.h) against the dense restatement
(tests/tsdf_ref.py) on the synthetic sphere with holes and a depth step: the
field masked to the seed bricks and their neighbours gives the dense mesh to
the bit in every array.  And, where the library loads, every refusal of the new
entry (status codes before any device call).  No GPU.

A brick grid of more than 2^28 bricks has no case: 4096 voxels per side give
512 x 512 x 1024 = 2^28 bricks exactly, so the dims limit refuses first and
the entry's brick-count check cannot be reached from outside."""
import ctypes as C

import numpy as np
import pytest

import tsdf_ref  # tests/tsdf_ref.py
import tsdf_sparse_ref  # tests/tsdf_sparse_ref.py

W, H, VIEWS = 128, 96, 6
MESH_KEYS = ("xyz", "normals", "rgb", "confidence", "faces")

# (origin, voxel, dims, min_weight): around the visible front; reaching toward
# the cameras (most bricks empty, free space known in front of the surface),
# twice; a finer grid
BOXES = [
    ((-1.15, -1.15, 2.85), 0.05, (46, 46, 28), 1),
    ((-1.22, -1.06, 0.45), 0.04, (61, 53, 75), 1),
    ((-1.22, -1.06, 0.45), 0.04, (61, 53, 75), 2),
    ((-1.17, -0.99, 2.0), 0.02, (117, 99, 90), 1),
]


@pytest.fixture(scope="module")
def views():
    from smvs_amd import synth
    inputs = synth.pipeline_inputs("sphere", W, H, VIEWS - 1, flen=1.2)
    cams = inputs["cams"]
    depths, _ = synth.depth_and_normal_maps(inputs["scene"], cams)
    rng = np.random.default_rng(11)
    for d in depths:
        d[rng.random(d.shape) < 0.03] = 0.0                              # 3 % holes
    depths[0][H // 5:H // 5 + 9, W // 4:W // 4 + 13] *= np.float32(0.8)   # a step
    for d in depths:
        d.setflags(write=False)
    return cams, depths, inputs["images"]


@pytest.fixture(scope="module")
def dense(views):
    """per box: the dense field and its mesh, computed once"""
    cams, depths, images = views
    out = []
    for origin, voxel, dims, mw in BOXES:
        F, Wt, col = tsdf_ref.field(cams, depths, images, origin, voxel, dims, min_weight=mw)
        mesh = tsdf_ref.surface(F, Wt, col, origin, voxel, len(cams))
        for a in (F, Wt, col) + tuple(mesh.values()):
            a.setflags(write=False)
        out.append((F, Wt, col, mesh))
    return out


@pytest.mark.parametrize("box", range(len(BOXES)))
def test_masked_field_gives_the_dense_mesh(views, dense, box):
    cams, depths, images = views
    origin, voxel, dims, mw = BOXES[box]
    F, Wt, col, want = dense[box]
    state = tsdf_sparse_ref.allocation(col, dims)
    assert state.shape == tsdf_sparse_ref.brick_dims(dims)[::-1]
    known = tsdf_sparse_ref._voxel_mask(state, F.shape)
    lost = int((~np.isnan(F) & ~known).sum())
    print("SPARSE-CPU dims=%s mw=%d bricks=%d seed=%d allocated=%d known-not-allocated=%d "
          "vertices=%d faces=%d" % (dims, mw, state.size, (state == 2).sum(),
                                    (state != 0).sum(), lost, len(want["xyz"]),
                                    len(want["faces"])))
    # not vacuous: something is left out
    assert 0 < (state == 2).sum() < (state != 0).sum() < state.size
    if box == 1:
        assert (state == 0).sum() > state.size // 2 and lost > 0
    got = tsdf_ref.surface(np.where(known, F, np.float32(np.nan)).astype(np.float32),
                           np.where(known, Wt, 0).astype(np.uint32),
                           np.where(known[..., None], col, 0).astype(np.uint32),
                           origin, voxel, len(cams))
    assert len(want["faces"]) > 100
    for k in MESH_KEYS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    # every inside corner is a seed
    with np.errstate(invalid="ignore"):
        assert np.all(col[..., 3][F < 0] > 0)


@pytest.mark.parametrize("box", [0, 2])
def test_sparse_order_is_a_permutation_of_the_dense_mesh(views, dense, box):
    cams, depths, images = views
    origin, voxel, dims, mw = BOXES[box]
    want = dense[box][3]
    got = tsdf_sparse_ref.fuse(cams, depths, images, origin, voxel, dims, min_weight=mw)
    cells = got["cells"]
    assert cells.dtype == np.int64 and len(cells) == len(want["xyz"])
    p = np.argsort(cells, kind="stable")
    assert np.all(np.diff(cells[p]) > 0)                       # strictly increasing
    assert np.array_equal(np.sort(p), np.arange(len(p)))       # a bijection
    assert not np.array_equal(p, np.arange(len(p)))            # and not the identity
    for k in ("xyz", "normals", "rgb", "confidence"):
        assert np.array_equal(got[k][p], want[k]), k
    # the cells are the dense active cells
    idx, _ = tsdf_sparse_ref._active_cells(dense[box][0])
    assert np.array_equal(cells[p], (idx[2].astype(np.int64) * dims[1] + idx[1]) * dims[0]
                          + idx[0])
    # the faces, relabelled to dense ids, are the dense faces as a set of rows
    rank = np.empty(len(p), np.int64)
    rank[p] = np.arange(len(p))
    relabelled = rank[got["faces"].astype(np.int64)]
    a = relabelled[np.lexsort(relabelled.T[::-1])]
    b = want["faces"].astype(np.int64)
    b = b[np.lexsort(b.T[::-1])]
    assert np.array_equal(a, b)
    assert got["stats"]["allocated_bricks"] == int((got["brick_state"] != 0).sum())
    assert got["stats"]["state_bytes"] == got["stats"]["allocated_bricks"] * 256 * 28


def test_field_window_over_the_whole_grid_is_the_field(views, dense):
    cams, depths, images = views
    origin, voxel, dims, mw = BOXES[2]
    F, Wt, col, _ = dense[2]
    gF, gW, gcol = tsdf_sparse_ref.field_window(cams, depths, images, origin, voxel, dims,
                                                (0, 0, 0), dims, min_weight=mw)
    assert np.array_equal(gF, F, equal_nan=True)
    assert np.array_equal(gW, Wt) and np.array_equal(gcol, col)
    # and a window of it is that part of the field
    lo, hi = (8, 16, 12), (40, 53, 60)
    wF, wW, wcol = tsdf_sparse_ref.field_window(cams, depths, images, origin, voxel, dims, lo,
                                                hi, min_weight=mw)
    sl = tuple(slice(lo[a], hi[a]) for a in (2, 1, 0))
    assert np.array_equal(wF, F[sl], equal_nan=True)
    assert np.array_equal(wW, Wt[sl]) and np.array_equal(wcol, col[sl])


def test_windowed_fusion_is_the_fusion(views):
    """fuse through a window that holds every seed with a brick to spare gives
    what fuse over the whole grid gives"""
    cams, depths, images = views
    origin, voxel, dims, mw = BOXES[1]
    whole = tsdf_sparse_ref.fuse(cams, depths, images, origin, voxel, dims, min_weight=mw)
    bz = np.nonzero((whole["brick_state"] == 2).any(axis=(1, 2)))[0]
    lo = (0, 0, int(bz.min() - 2) * 4)
    assert lo[2] > 0
    part = tsdf_sparse_ref.fuse(cams, depths, images, origin, voxel, dims, min_weight=mw,
                                window=(lo, dims))
    for k in MESH_KEYS + ("cells", "brick_state"):
        assert np.array_equal(part[k], whole[k]), k
    assert part["stats"] == whole["stats"]


# ------------------------------------------------------------------ refusals
@pytest.fixture(scope="module")
def lib():
    from smvs_amd import build as hip_build, _capi
    hip_build.build()
    return _capi.load()


def _call(lib, n=2, normals=True, depth=True, image=True, channels=3, volume=False,
          max_bricks=0, **changes):
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
    sopt = _capi.TsdfSparseOptions()
    sopt.max_bricks = max_bricks
    # a refused call may not touch the volume: one float stands for it
    one_f, one_w = (C.c_float * 1)(), (C.c_uint32 * 1)()
    handle = C.c_void_p(1)
    nv, nf = C.c_int64(-7), C.c_int64(-7)
    rc = lib.smvs_tsdf_fuse_sparse(0, arr if n > 0 else None, n, C.byref(opt), C.byref(sopt),
                                   None, one_f if volume else None, one_w if volume else None,
                                   None, C.byref(handle), C.byref(nv), C.byref(nf))
    return rc, handle.value


REFUSED = [
    dict(n=0), dict(n=-1),
    dict(voxel_size=0.0), dict(voxel_size=-0.1), dict(voxel_size=float("nan")),
    dict(voxel_size=float("inf")),
    dict(dims=(1, 8, 8)), dict(dims=(8, 8, 1)), dict(dims=(8, 8, 0)),
    dict(dims=(4097, 8, 8)), dict(dims=(8, 4097, 8)), dict(dims=(8, 8, 4097)),
    # tsdf / weight only within the dense entry's 2^27 voxels
    dict(dims=(1024, 1024, 129), volume=True), dict(dims=(4096, 4096, 4096), volume=True),
    dict(dims=(4096, 4096, 9), volume=True),
    dict(max_bricks=(1 << 23) + 1),
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
    handle = C.c_void_p(1)
    # no options, no handle pointer
    assert lib.smvs_tsdf_fuse_sparse(0, arr, 2, None, None, None, None, None, None,
                                     C.byref(handle), None, None) == -1
    assert handle.value is None
    assert lib.smvs_tsdf_fuse_sparse(0, arr, 2, None, None, None, None, None, None, None, None,
                                     None) == -1
    # the cells of no handle
    cells = (C.c_int64 * 4)()
    assert lib.smvs_tsdf_vertex_cells(None, cells) == -1
    if lib.smvs_device_count() < 1:
        # accepted arguments reach the device, and without one that is an error
        # of its own, not an argument error: sizes the dense entry refuses
        assert _call(lib, normals=False, cut_surfaces=0)[0] == -2
        assert _call(lib, dims=(4096, 16, 12))[0] == -2
        assert _call(lib, dims=(1025, 8, 8))[0] == -2
