"""CPU checks of the test-side PCG machinery: the SPD block-system builder and
its float64 CSR reference (tests/solver_systems.py), and the restatement of the
resident solver's plan (tests/solver_plans.py) pinned on hand-checked grids."""
import numpy as np
import pytest

import solver_plans as sp
import solver_systems as ss


# ------------------------------------------------------------------ builder
@pytest.mark.parametrize("stride,rows", [(2, 2), (5, 3), (7, 9)])
def test_csr_product_equals_the_block_product(stride, rows):
    s = ss.make_system(stride, rows, seed=stride * rows, holes=[1], isolated=[stride * rows - 1])
    y = np.random.default_rng(0).standard_normal(4 * s.num_nodes)
    ref = ss.block_product(s.H9, s.present, stride, y)
    assert np.allclose(s.csr() @ y, ref, rtol=0, atol=1e-13 * np.abs(ref).max())


@pytest.mark.parametrize("shift", [1.0, 1e-2, 1e-4])
def test_systems_are_symmetric_and_positive_definite(shift):
    holes = [0, 9, 23]
    s = ss.make_system(8, 6, seed=3, shift=shift, holes=holes, isolated=[30])
    A = s.csr().toarray()
    assert np.array_equal(A, A.T)
    keep = np.repeat(s.has_block, 4)
    np.linalg.cholesky(A[keep][:, keep])
    # holes: no block at all, zero g and P; isolated: the diagonal block only
    for n in holes:
        assert not s.present[n].any() and not s.g[4 * n:4 * n + 4].any()
        assert not s.P[n].any()
    assert s.present[30].tolist() == [0, 0, 0, 0, 1, 0, 0, 0, 0]
    # P holds the inverted diagonal blocks
    for n in np.flatnonzero(s.has_block):
        assert np.allclose(s.P[n].reshape(4, 4) @ s.H9[n, 4].reshape(4, 4), np.eye(4),
                           atol=1e-10)
    # the lower slots mirror the neighbours' upper slots
    N = s.num_nodes
    for n in range(N):
        for sl in range(9):
            if s.present[n, sl]:
                c = n + (sl // 3 - 1) * 8 + sl % 3 - 1
                assert s.present[c, 8 - sl]
                assert np.array_equal(s.H9[n, sl].reshape(4, 4), s.H9[c, 8 - sl].reshape(4, 4).T)


def test_conditioning_knob_and_g_modes():
    conds = []
    for shift in (1.0, 1e-2, 1e-4):
        A = ss.make_system(6, 6, seed=1, shift=shift).csr().toarray()
        conds.append(np.linalg.cond(A))
    assert conds[0] < conds[1] < conds[2]
    assert not ss.make_system(4, 4, g_mode="zero").g.any()
    g = ss.make_system(4, 4, g_mode="one", g_node=13).g.reshape(-1, 4)
    assert np.flatnonzero(np.abs(g).sum(1)).tolist() == [13]


def test_spsolve_and_oracle_cg_agree(oracle):
    s = ss.make_system(12, 9, seed=4, shift=1e-2, holes=[3, 50], isolated=[70])
    xs = s.spsolve()
    assert s.residual(xs) < 1e-12 * np.linalg.norm(s.g)
    x, it, info = ss.oracle_cg(oracle, s, 500, 1e-20 * np.dot(s.g, s.g), 0.0)
    assert info == 0 and it < 500
    assert np.linalg.norm(x - xs) < 1e-8 * np.linalg.norm(xs)


def test_oracle_system_goes_through_the_csr_path_unchanged(oracle):
    from smvs_amd import synth
    prob = synth.make_problem(96, 64, 3, 2, noise=0.004)
    orc = oracle.OracleProblem(prob["surf"], prob["views"])
    active = prob["surf"]["node_valid"].copy()
    active[::7] = 0
    ref = orc.gn_construct(active, 0.01)
    s = ss.system_from_oracle(ref, orc.node_stride)
    x = np.random.default_rng(2).standard_normal(4 * orc.num_nodes)
    y_orc = orc.spmv(ref["H9"], ref["present"], x)
    y_csr = s.csr() @ x
    assert np.linalg.norm(y_csr - y_orc) <= 1e-13 * np.linalg.norm(y_orc)
    A = s.csr()
    assert abs(A - A.T).max() == 0.0


# ---------------------------------------------------------- plan restatement
def test_lds_layout_hand_checked():
    # resident_lds_layout(30, 17, false): tile 32 x 19 x 4 + yl 2040 + P 4 x 2040
    # + rim (90 + 51) x 16 + x 2040 + b 2040 + 96 doubles of sums, flags, bits
    assert sp.lds_doubles(30, 17, False) == 2432 + 2040 + 8160 + 2256 + 2040 + 2040 + 96
    # one-exchange: P in three planes, r, no b, the halo ring of 2 x 32 + 2 x 17
    ring = 98
    assert sp.lds_doubles(30, 17, True) == (2432 + 2040 + 6120 + 2040 + 2256 + 2040
                                            + ring * 24 + (ring + 1) // 2 + 96)


@pytest.mark.parametrize("grid,ref,one", [
    ((480, 270), (30, 17), (30, 17)),     # 1920x1080 at scale 2: 256 tiles
    ((6, 4000), (6, 80), (8, 58)),        # 50 tiles vs 69
    ((2, 500), (6, 77), (8, 56)),
    ((500, 2), (125, 2), (100, 2)),
    ((2, 2), (47, 2), (47, 2)),
    ((256, 512), (16, 32), (16, 32)),
    ((8192, 16), (32, 16), (32, 16)),
    ((362, 362), None, None),             # 131,044 nodes and no tiling
    ((130, 1000), None, None),
    ((8193, 16), None, None),
])
def test_choose_tiling_hand_checked(grid, ref, one):
    assert sp.choose_tiling(*grid, False) == ref
    assert sp.choose_tiling(*grid, True) == one


def test_plan_rules():
    # AUTO: reference order on one tile, the one-exchange solver beyond
    assert not sp.plan(2, 2, "auto").one and sp.plan(2, 2, "auto").tiles == 1
    p = sp.plan(6, 4000, "auto")
    assert p.one and (p.tw, p.th, p.tiles) == (8, 58, 69)
    p = sp.plan(6, 4000, "resident_ref")
    assert not p.one and (p.tw, p.th, p.tiles) == (6, 80, 50)
    assert sp.plan(480, 270, "auto").tiles == 256
    # the streaming kernels: by request, no tiling, max_iterations <= 1, or
    # more epochs than the 16-bit tags count
    assert not sp.plan(8, 8, "streaming").resident
    assert not sp.plan(362, 362, "auto").resident
    assert not sp.plan(362, 362, "resident_ref").resident
    for mi, res in [(0, False), (1, False), (2, True), (32767, True), (32768, False)]:
        assert sp.plan(8, 8, "auto", max_iterations=mi).resident == res


def test_narrow_tiles_never_fit_the_lds():
    """tw = 4 and tw = 5 are in choose_tiling's loop but no th within eight
    rows of 512 / tw fits 160 KB, for either solver: the narrowest tiles the
    plan can pick are 6 wide (reference order) and 8 wide (one exchange).
    (If the LDS carve shrinks, tw = 4 becomes reachable and this fails: the
    shape list of the GPU module then needs a tw = 4 grid.)"""
    for one, narrowest in ((False, 6), (True, 8)):
        for tw in range(4, narrowest):
            th = sp.RES_THREADS // tw
            for t2 in range(th, th - 9, -1):
                assert sp.lds_doubles(tw, t2, one) * 8 > sp.RES_LDS_BYTES
        th = sp.RES_THREADS // narrowest
        assert any(sp.lds_doubles(narrowest, t2, one) * 8 <= sp.RES_LDS_BYTES
                   for t2 in range(th, th - 9, -1))


def test_plan_shapes_cover_every_class():
    """The GPU module's grid list reaches every plan class under both
    resident-capable solvers (delete a shape and this names what is lost)."""
    from test_gpu_solver_plans import PLAN_SHAPES
    for solver in ("auto", "resident_ref"):
        missing = sp.REQUIRED_CLASSES - sp.coverage(PLAN_SHAPES, solver)
        assert not missing, (solver, sorted(missing))

