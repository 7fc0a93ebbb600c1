"""The definition of the persistent brick-sparse fusion volume (the comment of
smvs_tsdf_sparse_volume_create in include/smvs_hip.h) restated in numpy with
explicit state, on top of tests/tsdf_ref.py (the field's seeds, the surface),
tests/tsdf_sparse_ref.py (bricks, the dilation, the sparse order) and
tests/tsdf_volume_ref.py (continuing the sums), which stay as they are.

A state is a dict: the grid (origin, voxel_size, dims, trunc), max_bricks,
seeds and slots (bz, by, bx) bool, birth (bz, by, bx) int64 (-1 without a
slot), the sums S (nz, ny, nx) float32, W uint32 and rgbc (nz, ny, nx, 4)
uint32 kept on the whole grid (zero outside the bricks with slots: a voxel's
sums depend on no other voxel, so summing everywhere and masking is summing on
the slots alone) and n_views.  mark and integrate return a new state and leave
their argument alone.  As in tsdf_ref.py the inputs are the PREPARED maps: the
cut maps of the batch, or the depth maps where nothing is cut."""
import numpy as np

import tsdf_ref  # tests/tsdf_ref.py
import tsdf_sparse_ref as sparse  # tests/tsdf_sparse_ref.py
import tsdf_volume_ref as dense  # tests/tsdf_volume_ref.py

f32 = np.float32
STATE_BYTES_PER_BRICK = 256 * 24
DEFAULT_MAX_BRICKS = 1 << 20


class OverBudget(Exception):
    """SMVS_ERR_NOMEM: the dilation of the would-be seeds has `need` bricks"""

    def __init__(self, need):
        super().__init__("the surface needs %d bricks" % need)
        self.need = need


def create(origin, voxel_size, dims, trunc=0, max_bricks=0):
    state = dense.create(origin, voxel_size, dims, trunc)
    bx, by, bz = sparse.brick_dims(dims)
    state.update(max_bricks=max_bricks if max_bricks > 0 else DEFAULT_MAX_BRICKS,
                 seeds=np.zeros((bz, by, bx), bool), slots=np.zeros((bz, by, bx), bool),
                 birth=np.full((bz, by, bx), -1, np.int64))
    return state


def dilation(seeds):
    """the seed bricks and their up to 26 neighbours"""
    return sparse._state_of_seed_bricks(seeds) != 0


def list_seeds(state, cams, cut_maps):
    """smvs_tsdf_fuse_sparse's seed rule on one list: the bricks that hold a
    voxel where some view of the list passes steps 1-6 with sdf <= trunc"""
    blind = [np.zeros(np.shape(m) + (1,), np.uint8) for m in cut_maps]
    _, _, col = tsdf_ref.field(cams, cut_maps, blind, state["origin"], state["voxel_size"],
                               state["dims"], state["trunc"])
    return sparse._seed_bricks(col[..., 3], state["seeds"].shape)


def mark(state, cams, cut_maps):
    seeds = state["seeds"] | list_seeds(state, cams, cut_maps)
    need = int(dilation(seeds).sum())
    if need > state["max_bricks"]:
        raise OverBudget(need)
    out = dict(state)
    out["seeds"] = seeds
    return out


def integrate(state, cams, cut_maps, images, grow=True):
    if grow:
        state = mark(state, cams, cut_maps)
    want = dilation(state["seeds"])
    if int(want.sum()) > state["max_bricks"]:
        raise OverBudget(int(want.sum()))
    fresh = want & ~state["slots"]
    slots = state["slots"] | fresh
    birth = np.where(fresh, state["n_views"], state["birth"])
    summed = dense.integrate(state, cams, cut_maps, images)
    mask = sparse._voxel_mask(slots, summed["S"].shape)
    out = dict(state)
    out.update(slots=slots, birth=birth, n_views=summed["n_views"],
               S=np.where(mask, summed["S"], f32(0)).astype(f32),
               W=np.where(mask, summed["W"], 0).astype(np.uint32),
               rgbc=np.where(mask[..., None], summed["rgbc"], 0).astype(np.uint32))
    return out


def stats(state):
    want = dilation(state["seeds"])
    n = int(state["slots"].sum())
    return {"bricks": state["slots"].size, "seed_bricks": int(state["seeds"].sum()),
            "allocated_bricks": n, "pending_bricks": int((want & ~state["slots"]).sum()),
            "late_bricks": int((state["birth"] > 0).sum()),
            "state_bytes": n * STATE_BYTES_PER_BRICK, "n_views": state["n_views"]}


def _slot_major(a, slots):
    """a (nz, ny, nx, ...) -> (n, 256, ...) over the bricks with slots in linear
    brick order, zero in the lanes outside the grid"""
    bz, by, bx = slots.shape
    full = np.zeros((bz * 4, by * 8, bx * 8) + a.shape[3:], a.dtype)
    full[:a.shape[0], :a.shape[1], :a.shape[2]] = a
    tail = tuple(range(6, 6 + a.ndim - 3))
    bricks = full.reshape((bz, 4, by, 8, bx, 8) + a.shape[3:]).transpose((0, 2, 4, 1, 3, 5) + tail)
    return bricks[slots].reshape((-1, 256) + a.shape[3:])


def checkpoint(state):
    """what smvs_tsdf_sparse_volume_download gives"""
    slots = state["slots"]
    return {"brick_state": sparse._state_of_seed_bricks(state["seeds"]),
            "list": np.nonzero(slots.reshape(-1))[0].astype(np.uint32),
            "birth": state["birth"][slots].astype(np.uint32),
            "S": _slot_major(state["S"], slots), "W": _slot_major(state["W"], slots),
            "rgbc": _slot_major(state["rgbc"], slots), "n_views": state["n_views"]}


def extract(state, min_weight=0):
    """smvs_tsdf_sparse_volume_extract -> the dict of tsdf_sparse_ref.fuse, the
    stats being this volume's"""
    mask = sparse._voxel_mask(state["slots"], state["S"].shape)
    F = np.where(mask, dense.field(state, min_weight), f32(np.nan)).astype(f32)
    with np.errstate(invalid="ignore", divide="ignore"):
        mesh = tsdf_ref.surface(F, state["W"], state["rgbc"], state["origin"],
                                state["voxel_size"], state["n_views"])
    idx, _ = sparse._active_cells(F)
    out, _ = sparse.reorder(mesh, tuple(x.astype(np.int64) for x in idx), state["dims"])
    out["brick_state"] = sparse._state_of_seed_bricks(state["seeds"])
    out["stats"] = stats(state)
    out["tsdf"] = F
    out["weight"] = state["W"]
    return out


def fuse_batches(batches, origin, voxel_size, dims, trunc=0, max_bricks=0, marks_first=True,
                 grow=None):
    """create; with marks_first every (cams, cut_maps, images) batch is marked,
    then every batch integrated (grow: default off after marks, else on)"""
    state = create(origin, voxel_size, dims, trunc, max_bricks)
    if marks_first:
        for cams, cut_maps, _ in batches:
            state = mark(state, cams, cut_maps)
    if grow is None:
        grow = not marks_first
    for cams, cut_maps, images in batches:
        state = integrate(state, cams, cut_maps, images, grow=grow)
    return state
