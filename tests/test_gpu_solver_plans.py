"""The PCG solvers on every plan class of the resident solver, through the C
ABI, against the oracle's ConjugateGradient::solve and a float64 sparse
solve.  Grids come from the plan restatement of tests/solver_plans.py (the
coverage of the list is checked on the CPU by test_solver_systems_cpu.py);
the profile counters confirm which solver ran (cg_resident against cg_spmv
launches).  Bounds: iteration count and info exact, x within 1e-9 relative
of the oracle's (as test_spmv_and_cg_match_oracle), within 1e-8 of spsolve
when a tight tolerance stops the solve."""

import numpy as np
import pytest

import solver_plans as sp
import solver_systems as ss

pytestmark = pytest.mark.gpu

SOLVERS = ["auto", "resident_ref", "streaming"]

# node grids (stride, rows); the classes each one reaches under auto / resident_ref
PLAN_SHAPES = [
    (2, 2),          # one tile, the smallest grid; th shortened (47 x 2)
    (2, 81),         # two tiles of 10 x 43
    (2, 500),        # 2 x N strip: 6 x 77 reference order, 8 x 56 one exchange
    (500, 2),        # N x 2 strip: 125 x 2 / 100 x 2
    (6, 4000),       # 50 tiles of 6 x 80 reference order, 69 of 8 x 58 one exchange
    (480, 270),      # 1920x1080 at scale 2: exactly 256 tiles of 30 x 17
    (11547, 11),     # last tile column holds one node (46 x 11, 252 tiles)
    (15, 8501),      # last tile row holds one node (15 x 34, 251 tiles)
    (362, 362),      # 131,044 nodes and no tiling: the streaming kernels
    (256, 512),      # 131,072 nodes, 256 tiles of 16 x 32
    (3, 43691),      # 131,073 nodes: the streaming kernels
]

# grids small enough for a sparse direct solve
SPSOLVE_NODES = 20000


def _rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


@pytest.fixture(scope="module")
def hip():
    import smvs_amd
    if smvs_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on a GPU")
    return smvs_amd


def _context(hip, stride, rows):
    surf = ss.flat_surface(stride, rows)
    ctx = hip.ViewContext(surf["width"], surf["height"], 1)
    ctx.set_surface(surf)
    ctx.profile(True)
    return ctx


def _launches(ctx):
    return {k: int(v[1]) for k, v in ctx.profile_get().items()}


def _gpu_solve(ctx, system, solver, max_it, etol, q_tol):
    """One solve of the uploaded system; checks the solver that ran against
    the plan restatement."""
    ctx.set_solver(solver)
    ctx.gn_upload(system.H9, system.g, system.P)
    ctx.profile_reset()
    it, info = ctx.cg_solve(max_it, etol, q_tol)
    x = ctx.cg_x()
    n = _launches(ctx)
    if sp.plan(system.stride, system.rows, solver, max_it).resident:
        assert n["cg_resident"] == 1 and n["cg_spmv"] == 0, (solver, max_it, n)
    else:
        assert n["cg_resident"] == 0, (solver, max_it, n)
        assert (n["cg_spmv"] > 0) == (max_it > 1), (solver, max_it, n)
    return x, it, info


def _stable(oracle, system, max_it, etol, q_tol, it_ref, trials=3):
    """The oracle's count does not move when g moves by 1e-12 relative (else
    the stop sits on a rounding edge, where a different association of the
    sums may legitimately end one iteration apart)."""
    rng = np.random.default_rng(7)
    for _ in range(trials):
        g = system.g * (1.0 + 1e-12 * rng.standard_normal(system.g.shape))
        tol = 0.01 * np.linalg.norm(g) if etol < 0 else etol
        if ss.oracle_cg(oracle, system, max_it, tol, q_tol, g=g)[1] != it_ref:
            return False
    return True


def _holes_and_empty_tile(stride, rows):
    """Holes inside the first tile and on its rim, a whole empty tile (of the
    AUTO plan) when there is more than one."""
    p = sp.plan(stride, rows, "auto")
    if not p.resident:
        p = sp.Plan(stride, rows, True, min(stride, 32), min(rows, 16))
    x0, y0, x1, y1 = p.tile_outline(0)
    holes = {((y0 + y1) // 2) * stride + (x0 + x1) // 2,   # inside
             y0 * stride + x1 - 1,                         # right rim
             (y1 - 1) * stride + x0}                       # bottom rim
    if p.tiles > 2:
        x0, y0, x1, y1 = p.tile_outline(p.tiles // 2)
        holes |= {y * stride + x for y in range(y0, y1) for x in range(x0, x1)}
    holes.discard(stride * rows - 1)
    return sorted(holes)


# the systems of every grid: (name, builder keywords, max_iterations, etol, q_tol)
def _cases(stride, rows):
    N = stride * rows
    rng = np.random.default_rng(N)
    iso = sorted(set(rng.integers(0, N, size=max(1, N // 500)).tolist()) | {N - 1})
    return [
        ("well", dict(shift=1.0), 200, -1.0, 1e-3),
        ("ill", dict(shift=1e-4), 200, -1.0, 1e-3),
        ("holes", dict(shift=1e-2, holes=_holes_and_empty_tile(stride, rows)), 200, -1.0, 1e-3),
        ("isolated", dict(shift=1e-2, isolated=iso), 200, -1.0, 1e-3),
        ("g_last_node", dict(shift=1e-2, g_mode="one", g_node=N - 1), 200, -1.0, 1e-3),
        ("max_iterations", dict(shift=1e-4), 4, 1e-30, 1e-12),
        ("tight", dict(shift=1.0), 400, "tight", 0.0),
    ]


def _case_ids():
    return ["%dx%d" % s for s in PLAN_SHAPES]


@pytest.mark.parametrize("shape", PLAN_SHAPES, ids=_case_ids())
def test_uploaded_systems_on_every_plan(hip, oracle, shape):
    stride, rows = shape
    N = stride * rows
    ctx = _context(hip, stride, rows)
    try:
        for name, kw, max_it, etol, q_tol in _cases(stride, rows):
            if name == "tight" and N > SPSOLVE_NODES:
                continue
            # a fixed scan of seeds: the first whose stop is not on a rounding edge
            for seed in range(16):
                system = ss.make_system(stride, rows, seed=seed, **kw)
                et = 2.5e-17 * float(system.g @ system.g) if etol == "tight" else etol
                tol = 0.01 * np.linalg.norm(system.g) if et < 0 else et
                xr, itr, infor = ss.oracle_cg(oracle, system, max_it, tol, q_tol)
                if name == "tight":
                    # the stop must be r.r < etol: without it the solve goes on
                    # (to the stop where Q no longer decreases, a rounding edge)
                    if ss.oracle_cg(oracle, system, max_it, 0.0, q_tol)[1] <= itr:
                        continue
                if _stable(oracle, system, max_it, et, q_tol, itr):
                    break
            else:
                pytest.fail("%s: no seed with a stable iteration count" % name)
            xs = system.spsolve() if name == "tight" else None
            for solver in SOLVERS:
                x, it, info = _gpu_solve(ctx, system, solver, max_it, et, q_tol)
                what = (shape, name, seed, solver)
                assert (it, info) == (itr, infor), (what, it, info, itr, infor)
                assert _rel(x, xr) < 1e-9, (what, _rel(x, xr))
                if name == "max_iterations":
                    assert (it, info) == (max_it, 1), what
                if name == "tight":
                    # stopped by r.r < etol: the true residual agrees
                    assert info == 0, what
                    assert _rel(x, xs) < 1e-8, (what, _rel(x, xs))
                    res = system.residual(x)
                    assert res * res < 1.001 * et, (what, res * res / et)
                if name in ("holes", "isolated"):
                    # nodes without a block keep x = 0
                    assert not x.reshape(-1, 4)[~system.has_block].any(), what
    finally:
        ctx.close()


@pytest.mark.parametrize("shape", [(2, 2), (2, 81), (480, 270)], ids=["2x2", "2x81", "480x270"])
def test_zero_gradient_follows_the_oracle(hip, oracle, shape):
    """g = 0: r.r = d.Ad = 0 and the reference's alpha is 0 / 0 -- the solve
    runs to max_iterations with x NaN wherever the oracle's is."""
    stride, rows = shape
    ctx = _context(hip, stride, rows)
    try:
        system = ss.make_system(stride, rows, seed=0, g_mode="zero")
        xr, itr, infor = ss.oracle_cg(oracle, system, 12, 0.0, 1e-3)
        for solver in SOLVERS:
            x, it, info = _gpu_solve(ctx, system, solver, 12, -1.0, 1e-3)
            assert (it, info) == (itr, infor), (solver, it, info, itr, infor)
            assert np.array_equal(np.isnan(x), np.isnan(xr)), solver
            assert np.array_equal(x[~np.isnan(x)], xr[~np.isnan(xr)]), solver
    finally:
        ctx.close()


@pytest.mark.parametrize("shape", [(2, 81), (6, 4000)], ids=["2x81", "6x4000"])
def test_max_iterations_edges(hip, oracle, shape):
    """max_iterations 1, 2, 3, 32767 and 32768: one "iteration" and x = 0 at
    1; the resident solver from 2 up to 32767; 32768 needs more exchange
    epochs than the 16-bit tags count and takes the streaming kernels."""
    stride, rows = shape
    ctx = _context(hip, stride, rows)
    try:
        system = ss.make_system(stride, rows, seed=1, shift=1e-3)
        for max_it in (1, 2, 3, 32767, 32768):
            tol = 0.01 * np.linalg.norm(system.g)
            xr, itr, infor = ss.oracle_cg(oracle, system, max_it, tol, 1e-3)
            for solver in SOLVERS:
                x, it, info = _gpu_solve(ctx, system, solver, max_it, -1.0, 1e-3)
                assert (it, info) == (itr, infor), (max_it, solver, it, info, itr, infor)
                assert _rel(x, xr) < 1e-9 if max_it > 1 else not x.any()
        assert sp.plan(stride, rows, "auto", 32767).resident
        assert not sp.plan(stride, rows, "auto", 32768).resident
    finally:
        ctx.close()


# ---------------------------------------------------------------------------
# sparse active sets through the product path: gn_construct picks the live
# tiles and halo slots of the resident solver
# ---------------------------------------------------------------------------
ACTIVE_SIZE = (640, 480, 3, 2)   # 161 x 121 nodes: 66 tiles of 27 x 11


def _patterns(p, valid):
    """Active sets on the tiles of plan `p` (AUTO and resident_ref agree here)."""
    stride, rows = p.stride, p.rows
    N = stride * rows
    grid = np.zeros((rows, stride), np.uint8)

    def tile(t, dx=0, dy=0):
        a = grid.copy()
        x0, y0, x1, y1 = p.tile_outline(t)
        a[y0 + dy:y1 + dy, x0 + dx:x1 + dx] = 1
        return a

    def node(t):
        a = grid.copy()
        x0, y0, x1, y1 = p.tile_outline(t)
        a[(y0 + y1) // 2, (x0 + x1) // 2] = 1
        return a

    inner = p.tiles_x + 1            # a tile off every border
    last_row = grid.copy(); last_row[p.tile_outline(p.tiles - 1)[1]:, :] = 1
    last_col = grid.copy(); last_col[:, p.tile_outline(p.tiles_x - 1)[0]:] = 1
    stripes_x = grid.copy(); stripes_x[:, ::7] = 1
    stripes_y = grid.copy(); stripes_y[::13, :] = 1
    checker = grid.copy()
    for t in range(p.tiles):
        if (t % p.tiles_x + t // p.tiles_x) % 2 == 0:
            checker |= tile(t)
    out = dict(node_interior=node(inner), node_last_tile=node(p.tiles - 1),
               tile_aligned=tile(inner), tile_offset=tile(inner, 1, 1),
               last_tile_row=last_row, last_tile_column=last_col,
               stripes_x7=stripes_x, stripes_y13=stripes_y, checkerboard=checker)
    valid = valid.reshape(rows, stride)
    return {k: (v & valid).reshape(N) for k, v in out.items()}


@pytest.fixture(scope="module")
def active_problem(hip, oracle):
    from smvs_amd import synth
    W, H, S, scale = ACTIVE_SIZE
    prob = synth.make_problem(W, H, S, scale, noise=0.01)
    surf = prob["surf"]
    p = sp.plan(surf["npx"] + 1, surf["npy"] + 1, "auto")
    assert p.resident and p.tiles > 16
    assert (p.tw, p.th) == (sp.plan(p.stride, p.rows, "resident_ref").tw,
                            sp.plan(p.stride, p.rows, "resident_ref").th)
    return prob, p, _patterns(p, surf["node_valid"])


PATTERNS = ["node_interior", "node_last_tile", "tile_aligned", "tile_offset",
            "last_tile_row", "last_tile_column", "stripes_x7", "stripes_y13",
            "checkerboard"]


@pytest.mark.parametrize("pattern", PATTERNS)
def test_sparse_active_sets_construct_and_solve(hip, oracle, active_problem, pattern):
    prob, p, patterns = active_problem
    W, H, S, _ = ACTIVE_SIZE
    act = patterns[pattern]
    assert act.any()
    orc = oracle.OracleProblem(prob["surf"], prob["views"])
    ref = orc.gn_construct(act, 0.01)
    tol = 0.01 * np.linalg.norm(ref["g"])
    xr, itr, infor = orc.cg_solve(ref["H9"], ref["present"], ref["P"], -ref["g"], 200,
                                  tol, 1e-3)
    system = ss.system_from_oracle(ref, orc.node_stride)
    assert _stable(oracle, system, 200, -1.0, 1e-3, itr), pattern
    ctx = hip.ViewContext(W, H, S)
    try:
        ctx.set_views(prob["views"])
        ctx.set_surface(prob["surf"])
        ctx.profile(True)
        for solver in SOLVERS:
            ctx.set_solver(solver)
            ctx.set_active(act)
            n = ctx.gn_construct(0.01)
            H9, g, P = ctx.gn_download()
            assert n == ref["active_patches"], (solver, n, ref["active_patches"])
            assert _rel(H9, ref["H9"]) < 1e-10 and _rel(g, ref["g"]) < 1e-10, solver
            assert np.all(H9[ref["present"] == 0] == 0.0), solver
            assert _rel(P, ref["P"]) < 1e-7, solver
            ctx.profile_reset()
            it, info = ctx.cg_solve(200, -1.0, 1e-3)
            x = ctx.cg_x()
            launches = _launches(ctx)
            assert (launches["cg_resident"] == 1) == (solver != "streaming"), (solver, launches)
            assert (it, info) == (itr, infor), (solver, it, info, itr, infor)
            assert _rel(x, xr) < 1e-9, (solver, _rel(x, xr))
            assert not x.reshape(-1, 4)[ref["present"][:, 4] == 0].any(), solver
    finally:
        ctx.close()


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("pattern", ["checkerboard", "last_tile_column"])
def test_gn_loop_from_a_sparse_active_set(hip, oracle, active_problem, pattern, solver):
    """smvs_gn_run_loop(reset_active = 0) from the pattern, against the
    oracle's loop (as test_gn_loop_from_a_partial_active_set)."""
    prob, p, patterns = active_problem
    W, H, S, _ = ACTIVE_SIZE
    active = patterns[pattern]
    orc = oracle.OracleProblem(prob["surf"], prob["views"])
    ctx = hip.ViewContext(W, H, S)
    try:
        ctx.set_solver(solver)
        ctx.set_views(prob["views"])
        ctx.set_surface(prob["surf"])
        ctx.set_active(active)
        stats = ctx.run_loop(0.01, max_newton_steps=4, reset_active=False)
        n_init = int(active.sum()); n_act = n_init; steps = 0; patch_steps = 0; its = 0
        act = active.copy()
        while steps < 4 and n_act > n_init // 20:
            steps += 1
            ref = orc.gn_construct(act, 0.01)
            patch_steps += ref["active_patches"]
            x, it, _ = orc.cg_solve(ref["H9"], ref["present"], ref["P"], -ref["g"], 200,
                                    0.01 * np.linalg.norm(ref["g"]), 1e-3)
            its += it
            act, n_act, _ = orc.update_and_reactivate(x, act)
        assert stats["newton_steps"] == steps
        assert stats["active_patch_steps"] == patch_steps
        assert stats["linear_iterations"] == its
        assert stats["final_active_nodes"] == n_act
        assert _rel(ctx.depth_map(), orc.depth_map()) <= 1e-5
    finally:
        ctx.close()
