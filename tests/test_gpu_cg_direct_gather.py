"""The one-exchange resident PCG's all-reduce in its two forms: the two-level
tree (SMVS_CG_GATHER=tree) and the direct gather (SMVS_CG_GATHER=direct: every
workgroup sums the members of all groups itself, grids of up to 5 groups of 16
tiles).  The totals are formed by the same additions on the same lanes, so
everything downstream must have the SAME BITS: array_equal, no tolerance.

The form is read once per process, so every variant runs in a fresh child
process (as test_compacted_solve_is_bit_identical_and_matches_oracle); one
child runs all the solves of its variant, the tests compare what they wrote.
Grids come from the plan restatement of tests/solver_plans.py: 17 tiles (a
second group of one member), 32, 33, 64 and 65 (a fifth group of one member:
the most a lane gathers; the cut-over was set by measurement at the 75 tiles
of a 1920 x 1080 view's scale 3, profiles/cg_direct_gather.txt)."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import solver_plans as sp
import solver_systems as ss

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (stride, rows) -> tiles of the AUTO plan
GRIDS = {17: (21, 385), 32: (60, 232), 33: (60, 209), 64: (68, 256), 65: (94, 246)}
SOLVE = dict(shift=1e-2)              # the systems: make_system(stride, rows, seed, **SOLVE)
LIMITS = (1, 2, 3)                    # max_iterations on the 33-tile grid


def test_grids_have_the_tilings_the_tests_are_about():
    for tiles, (stride, rows) in GRIDS.items():
        p = sp.plan(stride, rows, "auto")
        assert p.resident and p.one and p.tiles == tiles, p
        assert 8000 <= stride * rows <= 33000, p
    p = sp.plan(*COMPACT_GRID, "auto")
    assert p.resident and p.one and p.tiles == 64 and (p.tiles_x, p.tiles_y) == (8, 8), p


_UPLOAD_PROBE = r"""
import json, sys
import numpy as np
import torch  # noqa: F401  (one HIP runtime, see conftest.py)
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import smvs_amd
import solver_systems as ss
spec = json.load(open(sys.argv[2]))
out, arrays = [], {}
for grid in spec["grids"]:
    stride, rows = grid["shape"]
    surf = ss.flat_surface(stride, rows)
    ctx = smvs_amd.ViewContext(surf["width"], surf["height"], 1)
    ctx.set_surface(surf)
    ctx.profile(True)
    ctx.set_solver("auto")
    system = ss.make_system(stride, rows, seed=grid["seed"], **spec["system"])
    for i, (max_it, etol, q_tol) in enumerate(grid["solves"]):
        ctx.gn_upload(system.H9, system.g, system.P)
        ctx.profile_reset()
        it, info = ctx.cg_solve(max_it, etol, q_tol)
        name = "x_%d_%d" % (grid["tiles"], i)
        arrays[name] = ctx.cg_x()
        out.append(dict(tiles=grid["tiles"], solve=i, max_it=max_it, it=int(it), info=int(info),
                        x=name, launches={k: int(v[1]) for k, v in ctx.profile_get().items()}))
    ctx.close()
np.savez(sys.argv[3], **arrays)
print(json.dumps(out))
"""


def _run(probe, env_extra, args, tmp_path):
    env = dict(os.environ, SMVS_LOCK_DIR=str(tmp_path), **env_extra)
    res = subprocess.run([sys.executable, "-c", probe, ROOT] + [str(a) for a in args],
                         env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    return json.loads(res.stdout.strip().splitlines()[-1])


def _stable(oracle, system, max_it, q_tol, it_ref, trials=3):
    """The oracle's count does not move when g moves by 1e-12 relative (as
    test_gpu_solver_plans.py: else the stop sits on a rounding edge)."""
    rng = np.random.default_rng(7)
    for _ in range(trials):
        g = system.g * (1.0 + 1e-12 * rng.standard_normal(system.g.shape))
        if ss.oracle_cg(oracle, system, max_it, 0.01 * np.linalg.norm(g), q_tol, g=g)[1] != it_ref:
            return False
    return True


@pytest.fixture(scope="module")
def uploaded(oracle, tmp_path_factory):
    """Every uploaded solve under tree and under direct, and the oracle's
    answer to each: {variant: [records]}, {variant: arrays}, {(tiles, solve): oracle}."""
    tmp = tmp_path_factory.mktemp("direct_gather")
    grids, refs = [], {}
    for tiles, (stride, rows) in GRIDS.items():
        for seed in range(16):
            system = ss.make_system(stride, rows, seed=seed, **SOLVE)
            tol = 0.01 * np.linalg.norm(system.g)
            ref = ss.oracle_cg(oracle, system, 200, tol, 1e-3)
            if _stable(oracle, system, 200, 1e-3, ref[1]):
                break
        else:
            pytest.fail("%d tiles: no seed with a stable iteration count" % tiles)
        # the full solve, twice back to back on one context
        solves = [(200, -1.0, 1e-3), (200, -1.0, 1e-3)]
        refs[(tiles, 0)] = refs[(tiles, 1)] = ref
        if tiles == 33:
            for max_it in LIMITS:
                refs[(tiles, len(solves))] = ss.oracle_cg(oracle, system, max_it, tol, 1e-3)
                solves.append((max_it, -1.0, 1e-3))
        grids.append(dict(tiles=tiles, shape=[stride, rows], seed=seed, solves=solves))
    spec = tmp / "spec.json"
    spec.write_text(json.dumps(dict(grids=grids, system=SOLVE)))
    records, arrays = {}, {}
    for variant in ("tree", "direct"):
        records[variant] = _run(_UPLOAD_PROBE, {"SMVS_CG_GATHER": variant},
                                [spec, tmp / (variant + ".npz")], tmp)
        arrays[variant] = np.load(str(tmp / (variant + ".npz")))
    return records, arrays, refs


def _records(uploaded, tiles):
    records, arrays, refs = uploaded
    for t, d in zip(records["tree"], records["direct"]):
        assert (t["tiles"], t["solve"]) == (d["tiles"], d["solve"])
        if t["tiles"] == tiles:
            yield t, d, arrays["tree"][t["x"]], arrays["direct"][d["x"]], refs[(tiles, t["solve"])]


@pytest.mark.parametrize("tiles", sorted(GRIDS))
def test_direct_gather_gives_the_bits_of_the_tree(uploaded, tiles):
    """x, iteration count and info: tree == direct, bit for bit; the count and
    info are the oracle's, x within 1e-9 of it (the existing parity bound)."""
    seen = 0
    for t, d, xt, xd, (xr, itr, infor) in _records(uploaded, tiles):
        what = (tiles, t["solve"], t["max_it"])
        assert (t["it"], t["info"]) == (d["it"], d["info"]), what
        assert np.array_equal(xt, xd), what
        assert (d["it"], d["info"]) == (itr, infor), (what, d["it"], d["info"], itr, infor)
        if t["max_it"] > 1:
            assert np.linalg.norm(xd - xr) <= 1e-9 * np.linalg.norm(xr), what
        else:
            assert not xd.any(), what
        seen += 1
    assert seen == (2 + len(LIMITS) if tiles == 33 else 2)


def test_iteration_limits_use_both_epoch_parities(uploaded):
    """max_iterations 1, 2, 3 on the 33-tile grid: no, one and two exchanges of
    the one-exchange solver, so both parities of the lvl1 slots are reused."""
    got = [(t["max_it"], d["it"], d["info"]) for t, d, _, _, _ in _records(uploaded, 33)
           if t["solve"] >= 2]
    assert [g[0] for g in got] == list(LIMITS)
    for max_it, it, info in got:
        assert it == max_it, got


@pytest.mark.parametrize("tiles", sorted(GRIDS))
def test_two_solves_back_to_back_agree(uploaded, tiles):
    """The exchange area is not cleared between solves (the tags carry the
    solve id): the second solve on a context gives the first one's bits."""
    _, arrays, _ = uploaded
    for variant in ("tree", "direct"):
        a = arrays[variant]
        assert np.array_equal(a["x_%d_0" % tiles], a["x_%d_1" % tiles]), variant


def test_the_resident_solver_ran(uploaded):
    records, _, _ = uploaded
    for variant, recs in records.items():
        for r in recs:
            n = r["launches"]
            if r["max_it"] > 1:
                assert n["cg_resident"] == 1 and n["cg_spmv"] == 0, (variant, r)
            else:
                assert n["cg_resident"] == 0, (variant, r)


# ---------------------------------------------------------------------------
# compacted solves: tiles without an active node leave the launch, and the
# direct gather neither waits for them nor reads their slots
# ---------------------------------------------------------------------------
COMPACT_SIZE = (544, 736, 3, 2)      # 135 x 183 nodes: 8 x 8 tiles of 17 x 23
COMPACT_GRID = (135, 183)
ACTIVE_SETS = ["first_member_dead", "group_dead", "last_tile_only", "checkerboard"]


def _active_sets(p, valid):
    grid = np.zeros((p.rows, p.stride), np.uint8)

    def tiles(which):
        a = grid.copy()
        for t in which:
            x0, y0, x1, y1 = p.tile_outline(t)
            a[y0:y1, x0:x1] = 1
        return a

    every = range(p.tiles)
    out = dict(
        first_member_dead=tiles(t for t in every if t != 16),           # group 1 loses tile 16
        group_dead=tiles(t for t in every if not 32 <= t < 48),         # group 2 wholly dead
        last_tile_only=tiles([p.tiles - 1]),
        checkerboard=tiles(t for t in every if (t % p.tiles_x + t // p.tiles_x) % 2 == 0))
    valid = valid.reshape(p.rows, p.stride)
    return {k: (v & valid).reshape(-1).astype(np.uint8) for k, v in out.items()}


_COMPACT_PROBE = r"""
import json, sys
import numpy as np
import torch  # noqa: F401  (one HIP runtime, see conftest.py)
sys.path.insert(0, sys.argv[1])
import smvs_amd
from smvs_amd import synth
W, H, S, scale = json.loads(sys.argv[2])
prob = synth.make_problem(W, H, S, scale, noise=0.004)
sets = np.load(sys.argv[3])
out, arrays = {}, {}
ctx = smvs_amd.ViewContext(W, H, S)
ctx.set_views(prob["views"])
ctx.profile(True)
for name in sets.files:
    ctx.set_surface(prob["surf"])
    ctx.set_active(sets[name])
    ctx.profile_reset()
    stats = ctx.run_loop(0.01, max_newton_steps=3, reset_active=False)
    arrays["nodes_" + name] = ctx.get_nodes()
    arrays["active_" + name] = ctx.get_active()[0]
    out[name] = dict(stats={k: int(v) for k, v in stats.items()},
                     launches={k: int(v[1]) for k, v in ctx.profile_get().items()})
ctx.close()
np.savez(sys.argv[4], **arrays)
print(json.dumps(out))
"""


@pytest.fixture(scope="module")
def compacted(tmp_path_factory):
    from smvs_amd import synth
    tmp = tmp_path_factory.mktemp("direct_gather_compact")
    W, H, S, scale = COMPACT_SIZE
    surf = synth.make_problem(W, H, S, scale, noise=0.004)["surf"]
    assert (surf["npx"] + 1, surf["npy"] + 1) == COMPACT_GRID
    sets = _active_sets(sp.plan(*COMPACT_GRID, "auto"), surf["node_valid"])
    np.savez(str(tmp / "sets.npz"), **sets)
    replies, arrays = {}, {}
    for variant, extra in (("tree", {"SMVS_CG_GATHER": "tree"}),
                           ("direct", {"SMVS_CG_GATHER": "direct"}),
                           ("full_grid", {"SMVS_CG_GATHER": "direct", "SMVS_CG_COMPACT": "0"})):
        replies[variant] = _run(_COMPACT_PROBE, extra, [json.dumps(list(COMPACT_SIZE)),
                                tmp / "sets.npz", tmp / (variant + ".npz")], tmp)
        arrays[variant] = np.load(str(tmp / (variant + ".npz")))
    return sets, replies, arrays


@pytest.mark.parametrize("name", ACTIVE_SETS)
def test_compacted_solves_agree_in_every_form(compacted, name):
    """Nodes, Newton steps, CG iterations and the final active set: the same
    under tree, direct and the full grid (SMVS_CG_COMPACT=0); the resident
    solver ran every solve."""
    sets, replies, arrays = compacted
    assert sets[name].any()
    base = replies["tree"][name]
    assert base["stats"]["newton_steps"] >= 1 and base["stats"]["linear_iterations"] >= 1
    for variant in replies:
        r = replies[variant][name]
        assert r["launches"]["cg_resident"] > 0 and r["launches"]["cg_spmv"] == 0, (variant, r)
        assert r["stats"] == base["stats"], (variant, r["stats"], base["stats"])
        assert np.array_equal(arrays[variant]["nodes_" + name],
                              arrays["tree"]["nodes_" + name]), variant
        assert np.array_equal(arrays[variant]["active_" + name],
                              arrays["tree"]["active_" + name]), variant
