"""GPU parity of the adaptive-penalty SGM mode (DESIGN.md section 3.6,
SMVS_SGM_P2_ADAPTIVE: the reference's build without SSE, sgm_stereo.cc:310-346)
against the serial restatement tests/sgm_adaptive_reference.cc and the oracle's
unchanged pieces (cost volume, WTA, L/R check).  The path is integer: every
comparison is array_equal."""
import os
import subprocess
import sys

import numpy as np
import pytest

import sgm_adaptive_ref as ref  # tests/sgm_adaptive_ref.py

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hip():
    import smvs_amd
    if smvs_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on a GPU")
    return smvs_amd


@pytest.fixture(scope="module")
def scene_inputs():
    from smvs_amd import synth
    return synth.pipeline_inputs("sphere", 384, 256, 3, flen=1.2)


@pytest.fixture(scope="module")
def textured(scene_inputs):
    """Two textured u8 images of the synthetic scene at SGM scale (192 x 128)."""
    from smvs_amd import host
    return host.sgm_image(scene_inputs, 0, 1), host.sgm_image(scene_inputs, 1, 1)


def _crop_pair(textured, w, h):
    """A (main, neighbour) pair of w x h cut from the textured images, with a
    reprojection close to a shift (as tests/test_gpu_parity.py's SGM pairs)."""
    a, b = textured
    y0, x0 = (a.shape[0] - h) // 2, (a.shape[1] - w) // 2
    main = np.ascontiguousarray(a[y0:y0 + h, x0:x0 + w])
    nbr = np.ascontiguousarray(b[y0:y0 + h, x0:x0 + w])
    M = np.array([1.001, 0.002, 0.1, -0.001, 0.999, 0.2, 1e-6, -2e-6, 1.0], np.float32)
    t = np.array([-6.0, 0.3, 0.01], np.float32)
    return main, nbr, M, t


def _restated_run(oracle, main, nbr, M, t, lo, hi, D, p1, p2, literal):
    depths = oracle.sgm_depths(lo, hi, D)
    cost = oracle.sgm_cost_volume(main, nbr, M, t, depths)
    sgm = ref.aggregate(cost, main, p1, p2, literal=literal)
    depth, argmin = oracle.sgm_depth_from_volume(sgm, main, depths)
    return dict(cost=cost, sgm=sgm, depth=depth, argmin=argmin)


CASES = [
    (96, 64, 128, 6, 96),     # two lines per wave, every lane busy
    (71, 45, 64, 6, 96),      # two lines per wave, idle lanes; odd line counts
    (64, 40, 37, 6, 96),      # odd plane count: one launch per direction
    (80, 56, 64, 10, 300),    # penalty2 > 255: u16 volume with atomics
    (64, 40, 37, 10, 300),    # ... and with an odd plane count
    (50, 38, 38, 6, 96),      # planes not in fours: u16 volume with atomics
    (12, 9, 128, 6, 96),      # narrower than the two lines of a wave are long:
                              # most diagonals are shorter than a chunk
    (11, 9, 64, 6, 96),       # the smallest image the entry takes
    (48, 32, 64, 40, 20),     # penalty2 < penalty1: penalty2' = 60 everywhere
    (80, 56, 64, 170, 255),   # the largest penalties of the byte form
    (48, 32, 64, 171, 255),   # P1 * 3 / 2 = 256: one past it
    (12, 30, 5, 6, 96),       # one launch per direction on a portrait image: more
                              # entry-column diagonals than entry-row ones
    (11, 9, 5, 6, 96),        # ... and on the smallest image the entry takes
]


@pytest.mark.parametrize("w,h,D,p1,p2", CASES)
def test_adaptive_run_matches_restatement(hip, oracle, textured, w, h, D, p1, p2):
    """6. cost, sgm, argmin, depth of smvs_sgm_run_mode(ADAPTIVE) == restatement
    (literal j loop) + the oracle's WTA."""
    main, nbr, M, t = _crop_pair(textured, w, h)
    want = _restated_run(oracle, main, nbr, M, t, 1.0, 12.0, D, p1, p2, literal=True)
    got = hip.sgm_run(main, nbr, M, t, 1.0, 12.0, D, p1, p2, want_volumes=True,
                      adaptive_p2=True)
    assert np.array_equal(got["cost"], want["cost"])
    assert np.array_equal(got["sgm"], want["sgm"])
    assert np.array_equal(got["argmin"], want["argmin"])
    assert np.array_equal(got["depth"], want["depth"])
    # the same call without the volumes (S is then never formed in memory)
    lean = hip.sgm_run(main, nbr, M, t, 1.0, 12.0, D, p1, p2, adaptive_p2=True)
    assert np.array_equal(lean["depth"], want["depth"])
    assert np.array_equal(lean["argmin"], want["argmin"])
    if p2 >= p1 and p2 > p1 * 3 // 2 and w >= 40:
        # the image has texture and penalty2 has room above its floor: the mode
        # is not the constant one in disguise
        const = hip.sgm_run(main, nbr, M, t, 1.0, 12.0, D, p1, p2, want_volumes=True)
        assert not np.array_equal(const["sgm"], got["sgm"])


def test_adaptive_run_at_960x540x128(hip, oracle):
    """6. the flagship size (restatement in its closed form, which
    tests/test_sgm_adaptive_cpu.py shows equal to the literal loop)."""
    from smvs_amd import synth, host
    inputs = synth.pipeline_inputs("sphere", 960, 540, 1, flen=1.2)
    main = host.sgm_image(inputs, 0, 0)
    nbr = host.sgm_image(inputs, 1, 0)
    assert main.shape == (540, 960)
    M, t = host.view_reprojection(inputs, 0, 1)
    lo, hi = host.depth_range(inputs, 0)
    want = _restated_run(oracle, main, nbr, M, t, lo, hi, 128, 6, 96, literal=False)
    got = hip.sgm_run(main, nbr, M, t, lo, hi, 128, 6, 96, want_volumes=True,
                      adaptive_p2=True)
    assert np.array_equal(got["cost"], want["cost"])
    assert np.array_equal(got["sgm"], want["sgm"])
    assert np.array_equal(got["argmin"], want["argmin"])
    assert np.array_equal(got["depth"], want["depth"])
    assert (want["depth"] > 0).mean() > 0.2


_WAVE_PER_LINE = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import smvs_amd
from smvs_amd import synth, host
from oracle import pyoracle as oracle
import sgm_adaptive_ref as ref
inputs = synth.pipeline_inputs("sphere", 384, 256, 1, flen=1.2)
a, b = host.sgm_image(inputs, 0, 1), host.sgm_image(inputs, 1, 1)
main = np.ascontiguousarray(a[30:94, 40:136]); nbr = np.ascontiguousarray(b[30:94, 40:136])
M = np.array([1.001, 0.002, 0.1, -0.001, 0.999, 0.2, 1e-6, -2e-6, 1.0], np.float32)
t = np.array([-6.0, 0.3, 0.01], np.float32)
for D in (128, 36):
    depths = oracle.sgm_depths(1.0, 12.0, D)
    cost = oracle.sgm_cost_volume(main, nbr, M, t, depths)
    want = ref.aggregate(cost, main, 6, 96, literal=True)
    got = smvs_amd.sgm_run(main, nbr, M, t, 1.0, 12.0, D, 6, 96, want_volumes=True,
                           adaptive_p2=True)
    assert np.array_equal(got["sgm"], want), D
print("wave-per-line ok")
"""


def test_adaptive_wave_per_line_byte_form(hip, tmp_path):
    """6. the one-line-per-wave kernel in its byte form (SMVS_SGM_PATHS=wave,
    read once per process: a child process)."""
    script = tmp_path / "wave_per_line.py"
    script.write_text(_WAVE_PER_LINE)
    env = dict(os.environ, SMVS_SGM_PATHS="wave")
    out = subprocess.run(["timeout", "-k", "10", "300", sys.executable, str(script), ROOT],
                         env=env, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "wave-per-line ok" in out.stdout


@pytest.mark.parametrize("w,h,D,p1,p2", [(96, 64, 128, 6, 96), (71, 45, 64, 6, 96),
                                          (64, 40, 37, 6, 96), (80, 56, 64, 10, 300)])
def test_mode_0_through_the_new_entry_is_the_old_entry(hip, textured, w, h, D, p1, p2):
    """7. smvs_sgm_run_mode(CONSTANT) == smvs_sgm_run, byte for byte"""
    import ctypes as C
    from smvs_amd import _capi
    main, nbr, M, t = _crop_pair(textured, w, h)
    new = hip.sgm_run(main, nbr, M, t, 1.0, 12.0, D, p1, p2, want_volumes=True)
    lib = _capi.load()
    u8, fp = C.POINTER(C.c_uint8), C.POINTER(C.c_float)
    depth = np.zeros((h, w), np.float32)
    argmin = np.zeros((h, w), np.int32)
    cost = np.zeros((h, w, D), np.uint16)
    sgm = np.zeros((h, w, D), np.uint16)
    u16 = C.POINTER(C.c_uint16)
    _capi.check(lib.smvs_sgm_run(
        0, main.ctypes.data_as(u8), w, h, nbr.ctypes.data_as(u8), w, h, M.ctypes.data_as(fp),
        t.ctypes.data_as(fp), C.c_float(1.0), C.c_float(12.0), D, C.c_uint16(p1),
        C.c_uint16(p2), depth.ctypes.data_as(fp), argmin.ctypes.data_as(C.POINTER(C.c_int32)),
        cost.ctypes.data_as(u16), sgm.ctypes.data_as(u16)))
    assert new["depth"].tobytes() == depth.tobytes()
    assert np.array_equal(new["argmin"], argmin)
    assert np.array_equal(new["cost"], cost)
    assert np.array_equal(new["sgm"], sgm)


def _front_end_inputs(inputs):
    """The SGM-scale images, reprojections and depth ranges of the main view and
    its first two neighbours, as smvs_sgm_depth_for_view wants them."""
    from smvs_amd import host
    imgs = [host.sgm_image(inputs, k, 1) for k in range(3)]
    small = dict(inputs, images=imgs)
    nbs = []
    for k in (1, 2):
        Mf, tf = host.view_reprojection(small, 0, k)
        Mb, tb = host.view_reprojection(small, k, 0)
        nbs.append(dict(image=imgs[k], M_fwd=Mf, t_fwd=tf, M_bwd=Mb, t_bwd=tb,
                        range_main=host.depth_range(inputs, 0),
                        range_neighbor=host.depth_range(inputs, k)))
    return imgs[0], nbs


def _restated_front_end(oracle, main, nbs, p1=6, p2=96, D=128):
    maps = []
    for nb in nbs:
        fwd = _restated_run(oracle, main, nb["image"], nb["M_fwd"], nb["t_fwd"],
                            nb["range_main"][0], nb["range_main"][1], D, p1, p2, False)
        bwd = _restated_run(oracle, nb["image"], main, nb["M_bwd"], nb["t_bwd"],
                            nb["range_neighbor"][0], nb["range_neighbor"][1], D, p1, p2, False)
        maps.append(oracle.sgm_lr_check(fwd["depth"], bwd["depth"], nb["M_fwd"], nb["t_fwd"]))
    first, second = maps
    # app/smvsrecon.cc:366-377, as tests/test_oracle_sgm.py states it
    return np.where(second == 0, first, np.where(first == 0, second,
                    (first + second) * np.float32(0.5)))


@pytest.fixture(scope="module")
def front_end_map(oracle, scene_inputs):
    main, nbs = _front_end_inputs(scene_inputs)
    return _restated_front_end(oracle, main, nbs)


def test_depth_for_view_mode_matches_front_end_restated_from_parts(hip, oracle, scene_inputs,
                                                                   front_end_map):
    """8. smvs_sgm_depth_for_view_mode and ..._raw_mode, two neighbours"""
    main, nbs = _front_end_inputs(scene_inputs)
    want = front_end_map
    assert (want > 0).mean() > 0.3 and (want == 0).mean() > 0.01
    got = hip.sgm_depth_for_view(main, nbs, adaptive_p2=True)
    assert np.array_equal(got, want)
    raw = [dict(nb, image=scene_inputs["images"][k]) for nb, k in zip(nbs, (1, 2))]
    got_raw = hip.sgm_depth_for_view(scene_inputs["images"][0], raw, adaptive_p2=True,
                                     halvings=1)
    assert np.array_equal(got_raw, want)
    # mode 0 through the new entries is today's front end
    today = oracle.sgm_depth_for_view(scene_inputs, sgm_scale=1)
    assert np.array_equal(hip.sgm_depth_for_view(main, nbs), today)
    assert np.array_equal(hip.sgm_depth_for_view(scene_inputs["images"][0], raw, halvings=1),
                          today)
    assert not np.array_equal(today, want)


def test_host_mirror_honours_the_option(hip, oracle, scene_inputs, front_end_map):
    """9. SGMStereo::Options::adaptive_penalty2 through reconstruct_sgm_depth_for_view"""
    from smvs_amd import host
    got = host.sgm_depth(scene_inputs, sgm_scale=1, adaptive_penalty2=True)
    assert np.array_equal(got, front_end_map)
    off = host.sgm_depth(scene_inputs, sgm_scale=1)
    assert np.array_equal(off, oracle.sgm_depth_for_view(scene_inputs, sgm_scale=1))


def _stored(inputs, z):
    """What write_depth_to_view stores for the z-depth map z as "smvs-sgm"
    (MVE's ray-length convention), through the unchanged host mirror."""
    from smvs_amd import host
    host.optimize(inputs, regularization=0.01, num_iterations=1, min_scale=2, sgm_depth=z)
    return host.last_embeddings()["smvs-sgm"]


def test_reconstruct_scene_passes_the_option_down(hip, oracle, scene_inputs, tmp_path):
    """9. ReconSettings::sgm_adaptive_penalty2: the smvs-sgm embedding of the
    scene run is the front end of test 8 for the neighbours ViewSelection chose;
    without the option it is the embedding written today."""
    from smvs_amd import host, mve_scene
    inputs = scene_inputs
    scene = dict(views=[dict(id=i, flen=c.flen, rot=c.R, trans=c.t, width=384, height=256)
                        for i, c in enumerate(inputs["cams"])],
                 features=inputs["features"],
                 refs=[list(range(4))] * len(inputs["features"]))
    nb = host.select_neighbors(scene, 0, num_neighbors=3)
    assert len(nb) >= 2
    order = [0] + nb
    sel = dict(inputs, cams=[inputs["cams"][i] for i in order],
               images=[inputs["images"][i] for i in order], view_ids=order)
    main, nbs = _front_end_inputs(sel)
    want_on = _restated_front_end(oracle, main, nbs)
    want_off = oracle.sgm_depth_for_view(sel, sgm_scale=1)
    assert not np.array_equal(want_on, want_off)
    for name, flag, want in (("on", True, want_on), ("off", False, want_off)):
        d = str(tmp_path / name)
        os.makedirs(d)
        mve_scene.write_scene(d, inputs)
        kw = dict(sgm_adaptive_penalty2=True) if flag else {}
        done, skipped, _ = host.reconstruct_scene(d, view_ids=[0], num_neighbors=3,
                                                  min_neighbors=2, output_scale=2, **kw)
        assert done == [0] and skipped == 0
        got = mve_scene.load_mvei(os.path.join(d, "views", "view_0000.mve", "smvs-sgm.mvei"))
        assert got.shape == (128, 192)
        assert np.array_equal(got, _stored(sel, want)), name
