"""Re-activation with several pixels per thread (reactivate_kernel<FULL, K>,
csrc/reactivate.hip) against the CPU oracle, through the C ABI
(smvs_update_and_reactivate, smvs_get_active), on the smallest surfaces at which
the mapping of threads to pixels can go wrong:

* every patch size 4 .. 64 (scales 2 .. 6) on 5 x 3 patches whose grid starts at
  a non-zero (start_x, start_y): 16 pixels per patch are several patches per
  wave (and four lanes per patch at four pixels per thread), 4096 pixels are
  many waves per patch;
* 1 and 8 neighbours, a visibility mask with neighbours off per patch;
* two invalid patches (a corner one and an interior one) and an active set that
  leaves the last patch column without any active node;
* 15 patches in the stand-alone launch, which walks all patches: never a whole
  number of waves' patches where a wave holds several;
* the live list of the Newton loop (smvs_gn_run_loop from an uploaded active
  set, 5 x 3 patches of 16 and of 256 pixels): lists of 10 and then 7 patches,
  no multiple of the 4, 8 or 16 patches a wave holds, with the list length
  read on the device (launch-ahead loop) and known to the host (streaming
  solver, where the grid is sized for exactly that many patches);
* node deltas of very different size from node to node, scaled until the
  oracle re-activates between a quarter and three quarters of the live
  patches: where all or none move the comparison proves nothing;
* both full_optimization settings, and every value of SMVS_REACTIVATE_PIXELS in
  a process of its own.

Bars (the project's, tests/test_gpu_parity.py): identical active sets, nodes
within 1e-12, the mean shift of full optimisation within 1e-9 relative; the
Newton loop: the oracle loop's step, patch-step, iteration and active-node
counts and its depth map within 1e-5 relative.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALES = (2, 3, 4, 5, 6)
NEIGHBOURS = (1, 8)
NPX, NPY, START_X, START_Y = 5, 3, 7, 5
INVALID = (0, 1 * NPX + 2)          # the top-left corner, an interior patch
PIXELS = (1, 2, 4)                  # values of SMVS_REACTIVATE_PIXELS


def make_case(scale, n_subs):
    """Surface, views, start active set and node deltas (unscaled) of a case."""
    from smvs_amd import synth
    ps = 1 << scale
    width, height = START_X + NPX * ps + 9, START_Y + NPY * ps + 6
    main, subs = synth.ring_cameras(width, height, n_subs)
    Ms, ts = zip(*[synth.reprojection(main, s) for s in subs])
    K = main.K(np.float32)
    # (re-activation reads the cameras and the surface, not the images)
    views = dict(flen=float(K[0, 0]), inv_flen=float(main.Kinv(np.float32)[0, 0]),
                 grad=np.zeros((height, width, 2), np.float32),
                 subs=[(np.zeros((height, width, 2), np.float32),
                        np.zeros((height, width, 3), np.float32)) for _ in subs],
                 M=np.array(Ms), t=np.array(ts), shading=None, shading_grad=None)
    rng = np.random.default_rng(100 * scale + n_subs)
    iy, ix = np.meshgrid(np.arange(NPY + 1), np.arange(NPX + 1), indexing="ij")
    nodes = np.zeros((NPY + 1, NPX + 1, 4))
    nodes[..., 0] = 4.0 + 0.3 * np.sin(0.9 * ix + 0.4) * np.cos(0.7 * iy)
    nodes[..., 1] = 0.1 * rng.standard_normal(ix.shape)
    nodes[..., 2] = 0.1 * rng.standard_normal(ix.shape)
    nodes[..., 3] = 0.02 * rng.standard_normal(ix.shape)
    patch_valid = np.ones(NPX * NPY, np.uint8)
    patch_valid[list(INVALID)] = 0
    # some neighbours off per patch, never all of them
    vis = rng.integers(1, 1 << n_subs, NPX * NPY).astype(np.uint32) if n_subs > 1 \
        else np.ones(NPX * NPY, np.uint32)
    vis[patch_valid == 0] = 0
    pv = patch_valid.reshape(NPY, NPX)
    node_valid = np.zeros((NPY + 1, NPX + 1), np.uint8)
    node_valid[:-1, :-1] |= pv; node_valid[:-1, 1:] |= pv
    node_valid[1:, :-1] |= pv; node_valid[1:, 1:] |= pv
    surf = dict(scale=scale, npx=NPX, npy=NPY, start_x=START_X, start_y=START_Y,
                width=width, height=height, nodes=nodes.reshape(-1, 4),
                node_valid=node_valid.reshape(-1), patch_valid=patch_valid, patch_vis=vis)
    # the patches of the last column have no active node; one more node is off
    active = node_valid.copy()
    active[:, NPX - 1:] = 0
    active[1, 1] = 0
    # three decades of delta sizes from node to node
    delta = rng.standard_normal((NPY + 1, NPX + 1, 4)) * np.array([1.0, 0.3, 0.3, 0.1])
    delta *= 10.0 ** rng.uniform(-1.5, 1.5, ix.shape)[..., None]
    return dict(surf=surf, views=views, active=active.reshape(-1), delta=delta.reshape(-1))


def live_patches(case):
    a = case["active"].reshape(NPY + 1, NPX + 1)
    any_active = a[:-1, :-1] | a[:-1, 1:] | a[1:, :-1] | a[1:, 1:]
    return np.flatnonzero(case["surf"]["patch_valid"] & any_active.reshape(-1))


def moved_fraction(oracle, case, x):
    """Share of the live patches the oracle re-activates: each one alone on
    the surface (the oracle reports node flags, the union over the patches)."""
    live = live_patches(case)
    moved = 0
    for p in live:
        surf = dict(case["surf"])
        only = np.zeros_like(surf["patch_valid"])
        only[p] = 1
        surf["patch_valid"] = only
        _, n, _ = oracle.OracleProblem(surf, case["views"]).update_and_reactivate(
            x, case["active"])
        moved += 1 if n > 0 else 0
    return moved / live.size


@pytest.fixture(scope="module")
def cases(oracle):
    """Inputs and the oracle's answers, computed once."""
    out = {}
    for scale in SCALES:
        for n_subs in NEIGHBOURS:
            case = make_case(scale, n_subs)
            assert 0 < live_patches(case).size < case["surf"]["patch_valid"].sum()
            # the delta scale, walked down in quarter decades, at which the
            # share of the live patches that the oracle moves is nearest to one half
            frac = {}
            for e in range(0, -40, -1):
                frac[e] = moved_fraction(oracle, case, case["delta"] * 10.0 ** (0.25 * e))
                if frac[e] < 0.25:
                    break
            e = min(frac, key=lambda k: abs(frac[k] - 0.5))
            case["x"] = case["delta"] * 10.0 ** (0.25 * e)
            case["moved_fraction"] = frac[e]
            orc = oracle.OracleProblem(case["surf"], case["views"])
            case["new_active"], case["num_active"], _ = orc.update_and_reactivate(
                case["x"], case["active"])
            case["new_nodes"] = orc.nodes.copy()
            orc = oracle.OracleProblem(case["surf"], case["views"])
            _, _, case["mean_shift"] = orc.update_and_reactivate(
                case["x"], case["active"], full_optimization=True)
            out[(scale, n_subs)] = case
    return out


def run_case(hip, case, full):
    """-> active set, its count, nodes, mean shift on the device."""
    surf = case["surf"]
    ctx = hip.ViewContext(surf["width"], surf["height"], len(case["views"]["subs"]))
    ctx.set_views(case["views"])
    ctx.set_surface(surf)
    ctx.set_active(case["active"])
    ctx.cg_set_x(case["x"])
    n, mean, nan = ctx.update_and_reactivate(0.15, full)
    assert nan == 0
    active, cnt = ctx.get_active()
    nodes = ctx.get_nodes()
    ctx.close()
    assert n == cnt
    return active, cnt, nodes, mean


@pytest.fixture(scope="module")
def hip():
    import smvs_amd
    if smvs_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on a GPU")
    return smvs_amd


@pytest.mark.parametrize("n_subs", NEIGHBOURS)
@pytest.mark.parametrize("scale", SCALES)
def test_case_exercises_both_outcomes(cases, scale, n_subs):
    """Between a quarter and three quarters of the live patches re-activate in
    the oracle."""
    assert 0.25 <= cases[(scale, n_subs)]["moved_fraction"] <= 0.75


@pytest.mark.parametrize("n_subs", NEIGHBOURS)
@pytest.mark.parametrize("scale", SCALES)
def test_active_set_and_nodes_match_oracle(hip, cases, scale, n_subs):
    case = cases[(scale, n_subs)]
    active, cnt, nodes, _ = run_case(hip, case, False)
    assert cnt == case["num_active"]
    assert np.array_equal(active, case["new_active"])
    assert np.max(np.abs(nodes - case["new_nodes"])) <= 1e-12


@pytest.mark.parametrize("n_subs", NEIGHBOURS)
@pytest.mark.parametrize("scale", SCALES)
def test_full_optimization_mean_shift_matches_oracle(hip, cases, scale, n_subs):
    case = cases[(scale, n_subs)]
    active, _, nodes, mean = run_case(hip, case, True)
    assert abs(mean - case["mean_shift"]) <= 1e-9 * abs(case["mean_shift"])
    # the active set stays (depth_optimizer.cc:277-288)
    assert np.array_equal(active, case["active"])
    assert np.max(np.abs(nodes - case["new_nodes"])) <= 1e-12


# ------------------------------------------------------------ the Newton loop
LOOP_SCALES = (2, 4)
LOOP_SOLVERS = ("auto", "streaming")
LOOP_STEPS, LOOP_REG = 5, 0.01


def make_loop_case(scale):
    """A 5 x 3 surface on a textured sphere that fills the images, two invalid
    patches, two patches with a neighbour off, and a start active set that
    leaves the last patch column out."""
    from smvs_amd import synth
    ps, n_subs = 1 << scale, 3
    width, height = 6 * ps + 5, 4 * ps + 5
    main, subs = synth.ring_cameras(width, height, n_subs)
    scene = synth.SphereScene(seed=2000, radius=2.5,
                              px_size=3.0 / (main.flen * max(width, height)))
    planes = [synth.scale_planes(synth.render(scene, c), scale) for c in [main] + subs]
    Ms, ts = zip(*[synth.reprojection(main, s) for s in subs])
    K = main.K(np.float32)
    views = dict(flen=float(K[0, 0]), inv_flen=float(main.Kinv(np.float32)[0, 0]),
                 grad=planes[0][0], subs=[(g, h) for g, h in planes[1:]],
                 M=np.array(Ms), t=np.array(ts), shading=None, shading_grad=None)
    surf = synth.surface_from_depth(scene, main, subs, scale, noise=0.02)
    assert (surf["npx"], surf["npy"]) == (NPX, NPY) and surf["start_x"] > 0 < surf["start_y"]
    assert surf["patch_valid"].all()
    patch_valid = surf["patch_valid"].copy()
    patch_valid[list(INVALID)] = 0
    vis = surf["patch_vis"].copy()
    vis[3], vis[9] = 5, 6
    vis[patch_valid == 0] = 0
    pv = patch_valid.reshape(NPY, NPX)
    node_valid = np.zeros((NPY + 1, NPX + 1), np.uint8)
    node_valid[:-1, :-1] |= pv; node_valid[:-1, 1:] |= pv
    node_valid[1:, :-1] |= pv; node_valid[1:, 1:] |= pv
    surf.update(patch_valid=patch_valid, patch_vis=vis, node_valid=node_valid.reshape(-1))
    active = node_valid.copy()
    active[:, NPX - 1:] = 0
    active[1, 1] = 0
    return dict(surf=surf, views=views, active=active.reshape(-1))


def oracle_loop(oracle, case, full):
    """depth_optimizer.cc:219-304 step by step on the oracle -> the loop's
    statistics, the live-list lengths, the final active set and depth map."""
    orc = oracle.OracleProblem(case["surf"], case["views"])
    act = case["active"].copy()
    n_init = n_act = int(act.sum())
    steps = patch_steps = its = 0
    lists = []
    while steps < LOOP_STEPS and n_act > n_init // 20:
        steps += 1
        ref = orc.gn_construct(act, LOOP_REG)
        lists.append(ref["active_patches"])
        patch_steps += ref["active_patches"]
        x, it, _ = orc.cg_solve(ref["H9"], ref["present"], ref["P"], -ref["g"], 200,
                                0.01 * np.linalg.norm(ref["g"]), 1e-3)
        its += it
        new_act, n_new, mean = orc.update_and_reactivate(x, act, full)
        if full:
            if mean < 0.01:
                break
        else:
            act, n_act = new_act, n_new
    return dict(stats=[steps, its, patch_steps, n_act], lists=lists, active=act,
                depth=orc.depth_map())


def run_loop_case(hip, case, solver, full):
    """-> [newton_steps, linear_iterations, active_patch_steps,
    final_active_nodes], active set, nodes, depth map of the device's loop."""
    surf = case["surf"]
    ctx = hip.ViewContext(surf["width"], surf["height"], len(case["views"]["subs"]))
    ctx.set_solver(solver)
    ctx.set_views(case["views"])
    ctx.set_surface(surf)
    ctx.set_active(case["active"])
    st = ctx.run_loop(LOOP_REG, max_newton_steps=LOOP_STEPS, reset_active=False,
                      full_optimization=full)
    stats = [st["newton_steps"], st["linear_iterations"], st["active_patch_steps"],
             st["final_active_nodes"]]
    active, _ = ctx.get_active()
    nodes, depth = ctx.get_nodes(), ctx.depth_map()
    ctx.close()
    return stats, active, nodes, depth


@pytest.fixture(scope="module")
def loop_cases(oracle):
    out = {}
    for scale in LOOP_SCALES:
        case = make_loop_case(scale)
        case["ref"] = {full: oracle_loop(oracle, case, full) for full in (False, True)}
        out[scale] = case
    return out


def _rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


@pytest.mark.parametrize("scale", LOOP_SCALES)
def test_loop_case_has_ragged_live_lists(loop_cases, scale):
    """Several steps, and no live list fills the waves it is spread over: its
    length is no multiple of the patches a wave holds at any pixels per thread
    (at 256 pixels per patch a wave never holds a whole one)."""
    lists = loop_cases[scale]["ref"][False]["lists"]
    assert len(lists) >= 2 and lists[0] != lists[-1]
    for k in PIXELS:
        per_wave = max(1, 64 * k >> (2 * scale))
        assert per_wave == 1 or all(n % per_wave != 0 for n in lists), (k, lists)


@pytest.mark.parametrize("full", (False, True))
@pytest.mark.parametrize("solver", LOOP_SOLVERS)
@pytest.mark.parametrize("scale", LOOP_SCALES)
def test_newton_loop_on_a_short_live_list_matches_oracle(hip, loop_cases, scale, solver, full):
    case = loop_cases[scale]
    ref = case["ref"][full]
    stats, active, _, depth = run_loop_case(hip, case, solver, full)
    assert stats == ref["stats"]
    assert np.array_equal(active, ref["active"])
    assert _rel(depth, ref["depth"]) <= 1e-5


CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import smvs_amd
import test_gpu_reactivate_pixels as T
inputs = np.load(sys.argv[2])
out = {}
for scale in T.SCALES:
    for n_subs in T.NEIGHBOURS:
        case = T.make_case(scale, n_subs)
        case["x"] = inputs["x_%d_%d" % (scale, n_subs)]
        active, _, nodes, _ = T.run_case(smvs_amd, case, False)
        _, _, _, mean = T.run_case(smvs_amd, case, True)
        out["active_%d_%d" % (scale, n_subs)] = active
        out["nodes_%d_%d" % (scale, n_subs)] = nodes
        out["mean_%d_%d" % (scale, n_subs)] = np.float64(mean)
for scale in T.LOOP_SCALES:
    case = T.make_loop_case(scale)
    for solver in T.LOOP_SOLVERS:
        for full in (False, True):
            stats, active, nodes, depth = T.run_loop_case(smvs_amd, case, solver, full)
            tag = "loop_%d_%s_%d_" % (scale, solver, full)
            out[tag + "stats"] = np.array(stats)
            out[tag + "active"] = active
            out[tag + "nodes"] = nodes
            out[tag + "depth"] = depth
np.savez(sys.argv[3], **out)
"""


@pytest.fixture(scope="module")
def forced(hip, cases, tmp_path_factory):
    """Every case with each value of SMVS_REACTIVATE_PIXELS, each value in a
    process of its own (the library reads the switch once)."""
    tmp = tmp_path_factory.mktemp("reactivate_pixels")
    np.savez(str(tmp / "inputs.npz"),
             **{"x_%d_%d" % k: c["x"] for k, c in cases.items()})
    procs = {}
    for k in PIXELS:
        env = dict(os.environ, SMVS_REACTIVATE_PIXELS=str(k))
        procs[k] = subprocess.Popen(
            [sys.executable, "-c", CHILD, ROOT, str(tmp / "inputs.npz"),
             str(tmp / ("out_%d.npz" % k))], env=env, stdout=subprocess.PIPE,
            stderr=subprocess.STDOUT, text=True)
    out = {}
    try:
        for k, p in procs.items():
            text, _ = p.communicate(timeout=300)
            assert p.returncode == 0, text[-2000:]
            out[k] = dict(np.load(str(tmp / ("out_%d.npz" % k))))
    finally:
        # no child stays behind with the GPU open, whatever went wrong
        for p in procs.values():
            if p.poll() is None:
                p.kill()
            p.communicate()
    return out


@pytest.mark.parametrize("n_subs", NEIGHBOURS)
@pytest.mark.parametrize("scale", SCALES)
def test_every_pixels_per_thread_gives_the_same_active_set(forced, cases, scale, n_subs):
    case = cases[(scale, n_subs)]
    tag = "%d_%d" % (scale, n_subs)
    for k in PIXELS:
        assert np.array_equal(forced[k]["active_" + tag], case["new_active"]), k
        assert np.array_equal(forced[k]["active_" + tag], forced[PIXELS[0]]["active_" + tag]), k
        assert np.array_equal(forced[k]["nodes_" + tag], forced[PIXELS[0]]["nodes_" + tag]), k
        assert np.max(np.abs(forced[k]["nodes_" + tag] - case["new_nodes"])) <= 1e-12
        mean = float(forced[k]["mean_" + tag])
        assert abs(mean - case["mean_shift"]) <= 1e-9 * abs(case["mean_shift"]), k


@pytest.mark.parametrize("full", (False, True))
@pytest.mark.parametrize("solver", LOOP_SOLVERS)
@pytest.mark.parametrize("scale", LOOP_SCALES)
def test_every_pixels_per_thread_runs_the_same_newton_loop(forced, loop_cases, scale, solver,
                                                           full):
    """The live-list path (step_end_launch) under every value of the switch:
    the same loop bit for bit, and the oracle's."""
    ref = loop_cases[scale]["ref"][full]
    tag = "loop_%d_%s_%d_" % (scale, solver, full)
    first = forced[PIXELS[0]]
    for k in PIXELS:
        got = forced[k]
        assert list(got[tag + "stats"]) == ref["stats"], k
        assert np.array_equal(got[tag + "active"], ref["active"]), k
        assert _rel(got[tag + "depth"], ref["depth"]) <= 1e-5, k
        assert np.array_equal(got[tag + "active"], first[tag + "active"]), k
        assert np.array_equal(got[tag + "nodes"], first[tag + "nodes"]), k
