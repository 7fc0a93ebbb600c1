"""A Python restatement of how the PCG solve is planned, for the tests only.

csrc/cg_resident.hip decides on the host, before anything is launched, whether
a solve runs chip-resident (one workgroup per tile of the node grid) or on the
streaming kernels of csrc/cg.hip, which of the two resident solvers runs, and
on which tile shape.  This module restates those rules line by line so that
the tests can pick grids that land in every plan class and name the tiles of
a plan.  The constants are copied; the comments cite where they come from.
"""

# cg_resident.hip:59-61, 74
RES_THREADS = 512
RES_WAVES = RES_THREADS // 64
RES_MAX_BLOCKS = 256
RES_KINDS = 8
# choose_tiling: the LDS a tile may take (cg_resident.hip, `160 * 1024`)
RES_LDS_BYTES = 160 * 1024
# cg_resident_applies: the exchange tags carry the epoch in 16 bits
TAG_EPOCHS = 0xFFFF
# SMVS_REF_ORDER_TILES unset: AUTO runs the reference order on one tile
REF_ORDER_TILES = 1
# CUs of an MI355X: the resident solver's tile budget (min(CUs, RES_MAX_BLOCKS))
MI355X_CUS = 256


def lds_doubles(tw, th, one):
    """resident_lds_layout(tw, th, one).total (cg_resident.hip:1251-1284)."""
    tn = tw * th
    ring = 2 * (tw + 2) + 2 * th
    o = (tw + 2) * (th + 2) * 4           # direction tile with halo
    o += tn * 4                           # row sums from below
    o += (3 if one else 4) * tn * 4       # P: three or four planes
    o += tn * 4 if one else 0             # r (one-exchange)
    o += (3 * tw + 3 * th) * 16           # rim blocks
    o += tn * 4                           # x
    o += 0 if one else tn * 4             # b (two-exchange)
    if one:
        o += ring * 4 + ring * 16 + ring * 4 + (ring + 1) // 2   # halo r, P, q, ids
    o += RES_KINDS * RES_WAVES + RES_KINDS                # partial sums + results
    o += (RES_KINDS + 1) // 2                             # flags
    o += RES_KINDS + (RES_KINDS + 1) // 2                 # group mailbox
    o += (RES_WAVES + 1) // 2                             # wave tags
    o += RES_MAX_BLOCKS // 64                             # live bits
    return o


def tiles_of(stride, rows, tw, th):
    return -(-stride // tw) * -(-rows // th)


def choose_tiling(stride, rows, one, max_tiles=RES_MAX_BLOCKS):
    """choose_tiling (cg_resident.hip:2255-2285): (tw, th) or None."""
    best = None
    for tw in range(4, min(128, RES_THREADS) + 1):
        th = RES_THREADS // tw
        if th < 2:
            continue
        for t2 in range(th, max(2, th - 8) - 1, -1):
            tiles = tiles_of(stride, rows, tw, t2)
            if tiles > max_tiles:
                continue
            if lds_doubles(tw, t2, one) * 8 > RES_LDS_BYTES:
                continue
            waste = tiles * tw * t2 - stride * rows
            score = waste * 4 + tiles * (tw + t2)
            if best is None or score < best[0]:
                best = (score, tw, t2)
    return None if best is None else best[1:]


class Plan:
    """What smvs_cg_solve runs on a grid: `resident` False means the streaming
    kernels; otherwise tiles of tw x th, `one` the one-exchange solver."""

    def __init__(self, stride, rows, resident, tw=0, th=0, one=False):
        self.stride, self.rows = stride, rows
        self.resident, self.tw, self.th, self.one = resident, tw, th, one
        self.tiles_x = -(-stride // tw) if resident else 0
        self.tiles_y = -(-rows // th) if resident else 0
        self.tiles = self.tiles_x * self.tiles_y

    def tile_outline(self, t):
        """(x0, y0, x1, y1) node range of tile t (row-major, x1 / y1 exclusive)."""
        tx, ty = t % self.tiles_x, t // self.tiles_x
        return (tx * self.tw, ty * self.th, min(self.stride, (tx + 1) * self.tw),
                min(self.rows, (ty + 1) * self.th))

    def __repr__(self):
        if not self.resident:
            return "Plan(%dx%d streaming)" % (self.stride, self.rows)
        return "Plan(%dx%d %s %dx%d tiles=%d)" % (self.stride, self.rows,
            "one" if self.one else "ref", self.tw, self.th, self.tiles)


def plan(stride, rows, solver="auto", max_iterations=200, max_tiles=MI355X_CUS):
    """compute_resident_plan (cg_resident.hip:2332-2365) behind
    cg_resident_applies (cg_resident.hip:2369-2397)."""
    max_tiles = min(max_tiles, RES_MAX_BLOCKS)
    streaming = Plan(stride, rows, False)
    if solver == "streaming" or max_iterations <= 1:
        return streaming
    if 2 * max_iterations + 1 > TAG_EPOCHS:
        return streaming
    ref = choose_tiling(stride, rows, False, max_tiles)
    if ref is not None:
        if solver == "resident_ref" or tiles_of(stride, rows, *ref) <= REF_ORDER_TILES:
            return Plan(stride, rows, True, ref[0], ref[1], one=False)
    elif solver == "resident_ref":
        return streaming
    one = choose_tiling(stride, rows, True, max_tiles)
    if one is None:
        return streaming
    return Plan(stride, rows, True, one[0], one[1], one=True)


# ---------------------------------------------------------------- plan classes
def _ragged_one(stride, size):
    return stride % size == 1


def plan_classes(stride, rows, solver):
    """The classes of tests/test_gpu_solver_plans.py's list a grid falls in
    under one solver."""
    p = plan(stride, rows, solver)
    n = stride * rows
    out = set()
    if n == 131072:
        out.add("nodes_131072")
    if n == 131073:
        out.add("nodes_131073")
    if not p.resident:
        if n < RES_MAX_BLOCKS * RES_THREADS:
            out.add("streams_below_budget")
        return out
    if p.tiles == 1:
        out.add("one_tile")
    if p.tiles == 2:
        out.add("two_tiles")
    if p.tiles == RES_MAX_BLOCKS:
        out.add("tiles_256")
    if stride == 2 or rows == 2:
        out.add("strip_2")
    if p.tiles_x > 1 and _ragged_one(stride, p.tw):
        out.add("ragged_column_1")
    if p.tiles_y > 1 and _ragged_one(rows, p.th):
        out.add("ragged_row_1")
    if p.tw == (8 if p.one else 6):
        # the narrowest tile a plan can pick: tw = 4 and 5 never fit the LDS
        # (tests/test_solver_systems_cpu.py)
        out.add("tw_narrowest")
    if p.tw >= 100:
        out.add("tw_ge_100")
    if p.th < RES_THREADS // p.tw:
        out.add("th_shortened")
    if (plan(stride, rows, "auto").tiles > 1
            and choose_tiling(stride, rows, False) != choose_tiling(stride, rows, True)):
        # AUTO runs the one-exchange tiling, resident_ref another one
        out.add("ref_one_differ")
    return out


# every class the GPU module must reach, under `auto` and under `resident_ref`
REQUIRED_CLASSES = {
    "one_tile", "two_tiles", "tiles_256", "strip_2", "ragged_column_1",
    "ragged_row_1", "tw_narrowest", "tw_ge_100", "th_shortened", "ref_one_differ",
    "streams_below_budget", "nodes_131072", "nodes_131073",
}


def coverage(shapes, solver):
    """Plan classes the grids `shapes` reach under `solver`."""
    got = set()
    for stride, rows in shapes:
        got |= plan_classes(stride, rows, solver)
    return got
