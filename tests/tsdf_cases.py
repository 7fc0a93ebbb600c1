"""Inputs on which every rule of the volumetric fusion decides, and the tallies
that prove it, shared by tests/test_tsdf_cases_cpu.py (the restatement alone)
and tests/test_gpu_tsdf_cases.py (the device against the restatement).

The definition is the comment of smvs_tsdf_fuse in include/smvs_hip.h; tests/
tsdf_ref.py and tests/tsdf_sparse_ref.py restate it and stay as they are.  The
tallies walk the same steps once more, only to count where each (voxel, view)
pair leaves them, and check themselves against the restatement's W and F.

Case groups:
  rough     the sphere views with 15 % depth noise and 3 % holes and a band of
            0.5: a field whose cells take every inside/outside configuration
  exact     axis-aligned cameras and a dyadic grid, depths searched so that
            the comparisons of steps 2-8 are met with equality
  channels  four views with 1, 2, 3 and 4 channels in one call
  tiles     one rough case whose point blocks and allocated bricks both exceed
            one tile of the shared 64-bit scan
A case is a Case record.  Its depth maps are what the field reads when nothing
is cut; for the one case with cut=True the tests take the oracle's cut maps."""
import collections
import functools

import numpy as np

import tsdf_ref  # tests/tsdf_ref.py
import tsdf_sparse_ref  # tests/tsdf_sparse_ref.py

f32 = np.float32
BRICK = tsdf_sparse_ref.BRICK
POINT_BLOCK = 256         # grid points per block of the dense extraction
SCAN_TILE = 4096          # values per tile of the shared exclusive scan

Case = collections.namedtuple("Case", "name cams depths normals images box kw cut")

LEAVE = ("2 proj[2]<=0", "3 u<0", "3 v<0", "4 x>=width", "4 y>=height", "5 D==0",
         "6 sdf<-trunc", "7 clamped sdf>trunc", "8 coloured")
EQUALITIES = ("proj[2]==0", "u==0", "v==0", "sdf==-trunc", "sdf==trunc", "sdf==0")
PIXELS = ("integer u inside", "integer v inside", "last column", "last row")
NO_QUAD = ("low face", "last layer", "incomplete cell")


# ------------------------------------------------------------------- tallies
def tally_field(cams, maps, origin, voxel_size, dims, trunc=0, min_weight=0):
    """Where every (voxel, view) pair leaves steps 1-8, on the arithmetic of
    tsdf_ref.field -> dict
      leave   (n_views, 9) pairs per entry of LEAVE
      equal   pairs per entry of EQUALITIES, each counted where the step that
              compares the value is reached
      pixel   pairs that reach step 5 per entry of PIXELS
      weight  voxels with 0 < W < min_weight, W == min_weight, F == 0"""
    nx, ny, nz = (int(x) for x in dims)
    vs = f32(voxel_size)
    tr = f32(trunc) if trunc > 0 else f32(3.0) * vs
    mw = int(min_weight) if min_weight > 0 else 1
    shape = (nz, ny, nx)
    cx = np.broadcast_to(tsdf_ref._centres(origin, vs, nx, 0)[None, None, :], shape)
    cy = np.broadcast_to(tsdf_ref._centres(origin, vs, ny, 1)[None, :, None], shape)
    cz = np.broadcast_to(tsdf_ref._centres(origin, vs, nz, 2)[:, None, None], shape)
    leave = np.zeros((len(cams), len(LEAVE)), np.int64)
    equal = dict.fromkeys(EQUALITIES, 0)
    pixel = dict.fromkeys(PIXELS, 0)
    W = np.zeros(shape, np.uint32)
    for n, (cam, cut_map) in enumerate(zip(cams, maps)):
        h, w = cut_map.shape
        V = tsdf_ref.camera(cam, w, h)
        D = tsdf_ref.prepared_depth(V, cut_map)
        KR, t = V["KR"], V["t"]
        proj = []
        for r in range(3):
            s = f32(0) + KR[3 * r] * cx
            s = s + KR[3 * r + 1] * cy
            s = s + KR[3 * r + 2] * cz
            proj.append(s - t[r])
        step = np.full(shape, -1, np.int8)
        live = np.ones(shape, bool)

        def leaves(mask, code):
            step[live & mask] = code
            np.logical_and(live, ~mask, out=live)

        leaves(proj[2] <= 0, 0)
        reached3 = live.copy()
        den = np.where(live, proj[2], f32(1))
        u = proj[0] / den
        v = proj[1] / den
        leaves(u < 0, 1)
        leaves(v < 0, 2)
        leaves(u >= f32(w), 3)
        leaves(v >= f32(h), 4)
        xj = np.where(live, u, f32(0)).astype(np.int32)
        yj = np.where(live, v, f32(0)).astype(np.int32)
        reached5 = live.copy()
        d = D[yj, xj]
        leaves(d == 0, 5)
        reached6 = live.copy()
        sdf = d - proj[2]
        leaves(sdf < -tr, 6)
        leaves(sdf > tr, 7)
        step[live] = 8
        leave[n] = np.bincount(step.ravel(), minlength=len(LEAVE))
        W += (step >= 7).astype(np.uint32)
        equal["proj[2]==0"] += int((proj[2] == 0).sum())
        equal["u==0"] += int((reached3 & (u == 0)).sum())
        equal["v==0"] += int((reached3 & (v == 0)).sum())
        equal["sdf==-trunc"] += int((reached6 & (sdf == -tr)).sum())
        equal["sdf==trunc"] += int((reached6 & (sdf == tr)).sum())
        equal["sdf==0"] += int((reached6 & (sdf == 0)).sum())
        pixel["integer u inside"] += int((reached5 & (u == xj) & (xj > 0)).sum())
        pixel["integer v inside"] += int((reached5 & (v == yj) & (yj > 0)).sum())
        pixel["last column"] += int((reached5 & (xj == w - 1)).sum())
        pixel["last row"] += int((reached5 & (yj == h - 1)).sum())
    images = [np.zeros(m.shape, np.uint8) for m in maps]
    F, W_ref, _ = tsdf_ref.field(cams, maps, images, origin, voxel_size, dims, trunc, min_weight)
    assert np.array_equal(W, W_ref), "the tally walks other steps than the restatement"
    assert np.array_equal(np.isnan(F), W < mw)
    weight = {"0<W<min_weight": int(((W > 0) & (W < mw)).sum()),
              "W==min_weight": int((W == mw).sum()), "F==0": int((F == 0).sum())}
    return {"leave": leave, "equal": equal, "pixel": pixel, "weight": weight}


def m_of_config(config):
    """crossing edges of a cell whose corner c is inside when bit c is set"""
    return sum((config >> a & 1) != (config >> b & 1) for a, b, _ in tsdf_ref.EDGES)


def _cells(F):
    """-> corner values (nz-1, ny-1, nx-1, 8), complete, inside per corner, active"""
    f = np.stack([tsdf_ref._corner(F, c) for c in range(8)], -1)
    complete = ~np.isnan(f).any(axis=-1)
    with np.errstate(invalid="ignore"):
        inside = f < 0
    n_in = inside.sum(axis=-1)
    return f, complete, inside, complete & (n_in != 0) & (n_in != 8)


def _sign_change_edges(F, complete):
    """Per axis a: the grid points P (numpy index arrays k, j, i) whose edge to
    P + e_a has both ends known and one inside, whether P is the inside end,
    and per such edge the reason it gets no quad (-1: it gets one, else an
    index into NO_QUAD; the first that applies)"""
    shape = F.shape
    known = ~np.isnan(F)
    with np.errstate(invalid="ignore"):
        inside = known & (F < 0)
    out = []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        npa = 2 - a
        far_known = np.zeros(shape, bool)
        far_inside = np.zeros(shape, bool)
        dst = [slice(None)] * 3
        src = [slice(None)] * 3
        dst[npa] = slice(0, shape[npa] - 1)
        src[npa] = slice(1, shape[npa])
        far_known[tuple(dst)] = known[tuple(src)]
        far_inside[tuple(dst)] = inside[tuple(src)]
        edge = known & far_known & (inside != far_inside)
        at = np.nonzero(edge)
        idx = {0: at[2], 1: at[1], 2: at[0]}
        all_complete = np.ones(shape, bool)
        for ob, oc in ((-1, -1), (0, -1), (0, 0), (-1, 0)):
            off = [0, 0, 0]
            off[b], off[c] = ob, oc
            all_complete &= tsdf_ref._at_offset(complete, shape, off, False)
        low = (idx[b] == 0) | (idx[c] == 0)
        last = (idx[b] == shape[2 - b] - 1) | (idx[c] == shape[2 - c] - 1)
        reason = np.where(low, 0, np.where(last, 1, np.where(all_complete[at], -1, 2)))
        assert not (all_complete[at] & (low | last)).any()
        out.append((at, inside[at], reason))
    return out


def tally_surface(F):
    """What the extraction meets on a field F (nz, ny, nx) -> dict
      configs      the set of corner configurations (bit c: corner c inside) of
                   the active cells
      m            {crossing edges: active cells}
      active, incomplete_sign_change   cells; the latter have an inside and a
                   known outside corner and a NaN corner
      quads        (3, 2): per axis and orientation (0: P outside, 1: P inside)
      no_quad      (3, 2, 3): sign-change edges without a quad per NO_QUAD
      max_faces_per_edge, zero_normals, vertices, faces"""
    f, complete, inside, active = _cells(F)
    bits = (inside[active].astype(np.int64) << np.arange(8)).sum(axis=-1)
    configs = set(int(x) for x in np.unique(bits))
    crossing = np.zeros(len(bits), np.int64)
    for a, b, _ in tsdf_ref.EDGES:
        crossing += (bits >> a & 1) != (bits >> b & 1)
    m = {int(k): int(v) for k, v in zip(*np.unique(crossing, return_counts=True))}
    with np.errstate(invalid="ignore"):
        outside = f >= 0
    broken = ~complete & inside.any(axis=-1) & outside.any(axis=-1)
    quads = np.zeros((3, 2), np.int64)
    no_quad = np.zeros((3, 2, len(NO_QUAD)), np.int64)
    for a, (_, p_inside, reason) in enumerate(_sign_change_edges(F, complete)):
        for o in (0, 1):
            quads[a, o] = int(((reason < 0) & (p_inside == bool(o))).sum())
            for r in range(len(NO_QUAD)):
                no_quad[a, o, r] = int(((reason == r) & (p_inside == bool(o))).sum())
    zeros = np.zeros(F.shape, np.uint32)
    mesh = tsdf_ref.surface(F, zeros, np.zeros(F.shape + (4,), np.uint32), (0, 0, 0), 1.0, 1)
    assert len(mesh["faces"]) == 2 * quads.sum() and len(mesh["xyz"]) == active.sum()
    faces = mesh["faces"].astype(np.int64)
    most = 0
    if len(faces):
        e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
        e.sort(axis=1)
        most = int(np.unique(e[:, 0] * (len(mesh["xyz"]) + 1) + e[:, 1],
                             return_counts=True)[1].max())
    return {"configs": configs, "m": m, "active": int(active.sum()),
            "incomplete_sign_change": int(broken.sum()), "quads": quads, "no_quad": no_quad,
            "max_faces_per_edge": most,
            "zero_normals": int((~mesh["normals"].any(axis=1)).sum()),
            "vertices": len(mesh["xyz"]), "faces": len(faces)}


def tally_bricks(F, col, dims):
    """What the brick-sparse entry meets on the dense field F and colour sums
    col of a grid -> dict
      corner_span  {1, 2, 4, 8: active cells whose corners lie in that many bricks}
      quad_span    {1, 2, 4: quads whose four cells lie in that many bricks}
      halo_outside, halo_unallocated   voxels of the one-voxel halo around the
                   allocated bricks that are NaN because they lie outside the
                   grid / because their brick is not allocated
      dense_only_complete   cells the dense field completes, the sparse one not
      allocated, seeds, bricks; vertices_by_slot / quads_by_slot: per allocated
      brick in slot order the active cells / quads it owns"""
    dims = tuple(int(x) for x in dims)
    state = tsdf_sparse_ref.allocation(col, dims)
    known = tsdf_sparse_ref._voxel_mask(state, F.shape)
    Fs = np.where(known, F, f32(np.nan)).astype(f32)
    _, complete, _, active = _cells(Fs)
    _, dense_complete, _, dense_active = _cells(F)
    assert np.array_equal(active, dense_active)
    kk, jj, ii = np.nonzero(active)
    span = np.ones(len(ii), np.int64)
    for idx, side in zip((ii, jj, kk), BRICK):
        span *= 1 + ((idx + 1) % side == 0)
    corner_span = {s: int((span == s).sum()) for s in (1, 2, 4, 8)}
    bx, by, bz = tsdf_sparse_ref.brick_dims(dims)
    slot_of = np.cumsum(state.ravel() != 0) - 1
    n_alloc = int((state != 0).sum())

    def slots(i, j, k):
        return slot_of[(k // BRICK[2] * by + j // BRICK[1]) * bx + i // BRICK[0]]

    vertices_by_slot = np.bincount(slots(ii, jj, kk), minlength=n_alloc)
    quad_span = dict.fromkeys((1, 2, 4), 0)
    quads_by_slot = np.zeros(n_alloc, np.int64)
    for a, (at, _, reason) in enumerate(_sign_change_edges(Fs, complete)):
        b, c = (a + 1) % 3, (a + 2) % 3
        idx = {0: at[2][reason < 0], 1: at[1][reason < 0], 2: at[0][reason < 0]}
        s = (1 + (idx[b] % BRICK[b] == 0)) * (1 + (idx[c] % BRICK[c] == 0))
        for k in quad_span:
            quad_span[k] += int((s == k).sum())
        quads_by_slot += np.bincount(slots(idx[0], idx[1], idx[2]), minlength=n_alloc)
    # the halo: the brick grid's volume with one voxel around it
    full = (bz * BRICK[2], by * BRICK[1], bx * BRICK[0])
    in_grid = np.zeros(tuple(n + 2 for n in full), bool)
    in_grid[1:1 + dims[2], 1:1 + dims[1], 1:1 + dims[0]] = True
    alloc = np.zeros(in_grid.shape, bool)
    alloc[1:-1, 1:-1, 1:-1] = tsdf_sparse_ref._voxel_mask(state, full)
    outside, unallocated = ~in_grid, in_grid & ~alloc
    halo_outside = halo_unallocated = 0
    for k, j, i in zip(*np.nonzero(state)):
        box = (slice(k * BRICK[2], (k + 1) * BRICK[2] + 2),
               slice(j * BRICK[1], (j + 1) * BRICK[1] + 2),
               slice(i * BRICK[0], (i + 1) * BRICK[0] + 2))
        for which in (outside, unallocated):
            n = int(which[box].sum()) - int(which[box][1:-1, 1:-1, 1:-1].sum())
            if which is outside:
                halo_outside += n
            else:
                halo_unallocated += n
    return {"corner_span": corner_span, "quad_span": quad_span, "halo_outside": halo_outside,
            "halo_unallocated": halo_unallocated,
            "dense_only_complete": int((dense_complete & ~complete).sum()),
            "allocated": n_alloc, "seeds": int((state == 2).sum()), "bricks": bx * by * bz,
            "vertices_by_slot": vertices_by_slot, "quads_by_slot": quads_by_slot}


def block_counts(F):
    """Active cells and quads per block of POINT_BLOCK grid points in linear
    order: what the dense entry's scan runs over"""
    _, complete, _, active = _cells(F)
    nz, ny, nx = F.shape
    n_blocks = -(-F.size // POINT_BLOCK)
    kk, jj, ii = np.nonzero(active)
    vertices = np.bincount(((kk * ny + jj) * nx + ii) // POINT_BLOCK, minlength=n_blocks)
    quads = np.zeros(n_blocks, np.int64)
    for at, _, reason in _sign_change_edges(F, complete):
        k, j, i = (x[reason < 0] for x in at)
        quads += np.bincount(((k * ny + j) * nx + i) // POINT_BLOCK, minlength=n_blocks)
    return vertices, quads


# ------------------------------------------------------------- the rough group
ROUGH_TRUNC = 0.5
VOXEL = 0.06
ORIGIN = (-1.1, -0.9, 2.8)            # around the sphere's visible front (z = 3)
ODD = (37, 29, 23)                    # no side a multiple of a brick side
WHOLE = (40, 32, 24)                  # every side a whole number of bricks
ONE_IN = (33, 25, 17)                 # every side one voxel into its last brick
# reaches toward the cameras: free space the dense field knows, the sparse one
# does not allocate
DEEP = ((-1.22, -1.06, 0.45), 0.04, (61, 53, 75))
TILES = ((-1.12, -0.8, 2.9), 0.0165, (136, 96, 92))


@functools.lru_cache(maxsize=None)
def _sphere(n_views, w, h, last_size):
    from smvs_amd import synth
    base = synth.pipeline_inputs("sphere", w, h, max(n_views - 1, 1), flen=1.2)
    cams = base["cams"][:n_views]
    if last_size is not None:
        c = cams[-1]
        cams[-1] = synth.Camera(c.R, c.t, c.flen, last_size[0], last_size[1])
    depths, normals = synth.depth_and_normal_maps(base["scene"], cams)
    return cams, depths, normals


def rough_inputs(n_views, seed, last_size=None, channels=3, w=97, h=63):
    """The sphere views of tests/test_gpu_tsdf.py with depth * (1 + 0.15 N(0, 1)),
    3 % holes and the depth step in view 0.  channels: one count, or one per view."""
    cams, depths, normals = _sphere(n_views, w, h, last_size)
    depths = [d.copy() for d in depths]
    rng = np.random.default_rng(seed)
    for i in range(n_views):
        depths[i] *= (1.0 + 0.15 * rng.standard_normal(depths[i].shape)).astype(np.float32)
        depths[i][rng.random(depths[i].shape) < 0.03] = 0.0          # holes
    depths[0][h // 5:h // 5 + 9, w // 4:w // 4 + 13] *= np.float32(0.8)   # a step
    per_view = [channels] * n_views if np.isscalar(channels) else list(channels)
    images = [rng.integers(0, 256, d.shape if ch == 1 else d.shape + (ch,)).astype(np.uint8)
              for d, ch in zip(depths, per_view)]
    return list(cams), depths, list(normals), images


#        name                box                     views seed last size  min_weight cut
ROUGH = (("rough-odd-3v", (ORIGIN, VOXEL, ODD), 3, 11, None, 1, False),
         ("rough-whole-5v", (ORIGIN, VOXEL, WHOLE), 5, 12, None, 2, False),
         ("rough-one-in-mixed", (ORIGIN, VOXEL, ONE_IN), 3, 13, (80, 71), 2, False),
         ("rough-whole-3v", (ORIGIN, VOXEL, WHOLE), 3, 13, None, 1, False),
         ("rough-one-in-5v", (ORIGIN, VOXEL, ONE_IN), 5, 11, None, 1, False),
         ("rough-deep-3v", DEEP, 3, 12, None, 1, False),
         # (the cut keeps about one pixel in twenty of such maps: a field of
         # scattered columns, hardly a complete cell, one vertex and no face)
         ("rough-odd-5v-cut", (ORIGIN, VOXEL, ODD), 5, 11, None, 1, True))
ROUGH_NAMES = tuple(r[0] for r in ROUGH)
ROUGH_UNCUT = tuple(r[0] for r in ROUGH if not r[6])


def _rough(name):
    _, box, n_views, seed, last_size, min_weight, cut = ROUGH[ROUGH_NAMES.index(name)]
    cams, depths, normals, images = rough_inputs(n_views, seed, last_size)
    return Case(name, cams, depths, normals, images, box,
                dict(trunc=ROUGH_TRUNC, min_weight=min_weight), cut)


def _tiles():
    cams, depths, normals, images = rough_inputs(3, 12)
    return Case("tiles", cams, depths, normals, images, TILES,
                dict(trunc=ROUGH_TRUNC, min_weight=1), False)


def _channels():
    cams, depths, normals, images = rough_inputs(4, 14, channels=(1, 2, 3, 4))
    return Case("channels", cams, depths, normals, images, (ORIGIN, VOXEL, ODD),
                dict(trunc=ROUGH_TRUNC, min_weight=1), False)


def misread_channels(images, mistake):
    """The images a kernel with that mistake would in effect read, as inputs of
    the restatement: "4-as-grey" takes byte 0 of a 4-channel pixel for all
    three colours; "2-as-rgb" reads three consecutive bytes at a 2-channel
    pixel (its two and the next pixel's first; 0 behind the last)."""
    out = []
    for im in images:
        if mistake == "4-as-grey" and im.ndim == 3 and im.shape[2] == 4:
            im = np.ascontiguousarray(im[..., 0])
        elif mistake == "2-as-rgb" and im.ndim == 3 and im.shape[2] == 2:
            flat = np.concatenate([im.ravel(), np.zeros(1, np.uint8)])
            at = 2 * np.arange(im.shape[0] * im.shape[1])
            im = np.stack([flat[at], flat[at + 1], flat[at + 2]], -1).reshape(im.shape[:2] + (3,))
        out.append(im)
    return out


# ------------------------------------------------------------- the exact group
EXACT_VOXEL = 0.25
# dyadic, so that D = proj[2] +- trunc is a float, and no power of two, so
# that sdf / trunc rounds and the order of the sum S shows
EXACT_TRUNC = 0.375
EXACT_ORIGIN = (-1.125, -0.875, -0.125)   # centres x -1 .. 1, y -0.75 .. 1, z 0 .. 1.25
EXACT_DIMS = (9, 8, 6)
# the same voxels four, four and two indices up: x = 0 is the first voxel of the
# second brick, y = 0 the last of the first, the surface lies across a brick face
EXACT_SHIFT = (4, 4, 2)
# (width, height, centre): R = I, flen * max(w, h) = 8, principal points 8 / 4
EXACT_VIEWS = ((16, 8, (0.0, 0.0, 0.0)), (16, 8, (0.125, 0.125, 0.0)),
               (8, 16, (0.0, -0.25, 0.0)))
EXACT_PLANES = (1.1, 1.2, 1.3)            # about the z-depth of the views' base maps
# (view, voxel (i, j, k), sdf): the depth of the pixel the voxel projects to is
# searched so that the view's sdf at the voxel is exactly this.  The first
# three make F == 0 at voxel (4, 3, 4); the last makes its neighbour above it
# inside, so that an edge crosses at t = 0.
EXACT_TARGETS = ((0, (4, 3, 4), 0.25), (1, (4, 3, 4), -0.25), (2, (4, 3, 4), 0.0),
                 (0, (6, 3, 3), EXACT_TRUNC), (0, (2, 3, 4), -EXACT_TRUNC),
                 (1, (6, 5, 4), EXACT_TRUNC), (2, (4, 5, 4), -EXACT_TRUNC),
                 (1, (2, 2, 4), 0.0), (2, (4, 3, 5), -0.125))
# (view, pixel (x, y), z-depth): holes and depths far in front of the voxels
EXACT_PIXELS = ((0, (5, 5), 0.0), (1, (9, 2), 0.0), (2, (3, 9), 0.0),
                (0, (10, 5), 0.3), (1, (6, 6), 0.3), (2, (5, 6), 0.3))


def exact_depth(V, x, y, target, reach=64):
    """The ray-length depth at pixel (x, y) of view V whose prepared z-depth is
    exactly `target`: the prepared depth is a rounded product, so the
    neighbouring floats of target * length are tried in turn; None when none
    of them gives it"""
    if target == 0:
        return f32(0)
    _, length = tsdf_ref._pixel_rays(V)
    d = f32(np.float64(target) * np.float64(length[y, x]))
    below = above = d
    probe = np.zeros((V["h"], V["w"]), f32)
    for _ in range(reach):
        for cand in (below, above):
            probe[y, x] = cand
            if tsdf_ref.prepared_depth(V, probe)[y, x] == f32(target):
                return cand
        below = np.nextafter(below, f32(0))
        above = np.nextafter(above, f32(np.inf))
    return None


def _exact(shifted):
    from smvs_amd import synth
    shift = EXACT_SHIFT if shifted else (0, 0, 0)
    origin = tuple(o - s * EXACT_VOXEL for o, s in zip(EXACT_ORIGIN, shift))
    dims = tuple(n + s for n, s in zip(EXACT_DIMS, shift))
    rng = np.random.default_rng(21)
    cams, depths, images = [], [], []
    for n, (w, h, centre) in enumerate(EXACT_VIEWS):
        cam = synth.Camera(np.eye(3), -np.asarray(centre), 8.0 / max(w, h), w, h)
        V = tsdf_ref.camera(cam, w, h)
        _, length = tsdf_ref._pixel_rays(V)
        # (off the plane by up to 0.05 per pixel: the three views' values at a
        # voxel are then unrelated floats, and their sum depends on its order)
        plane = EXACT_PLANES[n] + 0.05 * rng.uniform(-1.0, 1.0, (h, w))
        depth = (plane.astype(f32) * length).astype(f32)
        for view, (x, y), z in EXACT_PIXELS:
            if view == n:
                depth[y, x] = exact_depth(V, x, y, z) if z == 0 else f32(z) * length[y, x]
        for view, voxel, sdf in EXACT_TARGETS:
            if view != n:
                continue
            c = [f32(EXACT_ORIGIN[a]) + (f32(voxel[a]) + f32(0.5)) * f32(EXACT_VOXEL)
                 for a in range(3)]
            p = [sum(V["KR"][3 * r + k] * c[k] for k in range(3)) - V["t"][r] for r in range(3)]
            x, y = int(p[0] / p[2]), int(p[1] / p[2])
            assert 0 <= x < w and 0 <= y < h, (view, voxel)
            d = exact_depth(V, x, y, float(p[2]) + sdf)
            assert d is not None, "no float depth gives view %d voxel %s sdf %r" % (
                view, voxel, sdf)
            depth[y, x] = d
        cams.append(cam)
        depths.append(depth)
        images.append(rng.integers(0, 256, (h, w) if n == 1 else (h, w, 3)).astype(np.uint8))
    normals = [np.zeros(d.shape + (3,), f32) for d in depths]
    return Case("exact-shifted" if shifted else "exact", cams, depths, normals, images,
                (origin, EXACT_VOXEL, dims), dict(trunc=EXACT_TRUNC, min_weight=1), False)


def exact_f0_voxel(case):
    """(k, j, i) of the voxel two views give +0.25 and -0.25 and one 0"""
    shift = EXACT_SHIFT if case.name == "exact-shifted" else (0, 0, 0)
    i, j, k = (v + s for v, s in zip(EXACT_TARGETS[0][1], shift))
    return k, j, i


# ------------------------------------------------------------------- the list
EXACT_NAMES = ("exact", "exact-shifted")
SMALL_NAMES = ROUGH_NAMES + EXACT_NAMES + ("channels",)
NAMES = SMALL_NAMES + ("tiles",)
UNCUT_NAMES = tuple(n for n in NAMES if n not in ROUGH_NAMES or n in ROUGH_UNCUT)


@functools.lru_cache(maxsize=None)
def get(name):
    if name in ROUGH_NAMES:
        case = _rough(name)
    elif name in EXACT_NAMES:
        case = _exact(name == "exact-shifted")
    else:
        case = {"channels": _channels, "tiles": _tiles}[name]()
    for group in (case.depths, case.normals, case.images):
        for a in group:
            a.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def field_of(name):
    """F, W, col of an uncut case by the restatement (computed once, read-only)"""
    c = get(name)
    assert not c.cut
    origin, voxel, dims = c.box
    out = tsdf_ref.field(c.cams, c.depths, c.images, origin, voxel, dims, **c.kw)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def restated(name, sparse=False):
    """tsdf_ref.fuse / tsdf_sparse_ref.fuse of an uncut case (once, read-only)"""
    c = get(name)
    assert not c.cut
    origin, voxel, dims = c.box
    ref = tsdf_sparse_ref if sparse else tsdf_ref
    out = ref.fuse(c.cams, c.depths, c.images, origin, voxel, dims, **c.kw)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out
