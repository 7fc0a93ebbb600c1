"""The device input scaling (smvs_rescale_half_gaussian, the input scaling of
app/smvsrecon.cc:621-650) against the oracle's and the host mirror's
rescale_half_size_gaussian<uint8_t> ([MVE-unverified] M29): identity, so every
comparison is np.array_equal."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# the smallest legal image, odd sizes (both right-hand clamps on one column),
# sizes just above a power of two (a partial tile and a partial dword end the
# rows); 515 -> 258 outputs crosses the one-channel tile of 256, 67 -> 34 rows
# the tile height of 16 twice
WIDTHS = (2, 3, 5, 129, 257, 515)
HEIGHTS = (2, 3, 7, 33, 67)


@pytest.fixture(scope="module")
def hip():
    import smvs_amd
    if smvs_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on a GPU")
    return smvs_amd


def _contents(w, h, c):
    rng = np.random.default_rng(1000 * w + 10 * h + c)
    ys, xs = np.mgrid[0:h, 0:w]
    yield "random", rng.integers(0, 256, (h, w, c)).astype(np.uint8)
    yield "all255", np.full((h, w, c), 255, np.uint8)
    yield "all0", np.zeros((h, w, c), np.uint8)
    # 0 / 255 checkerboards: quotients near .5
    for period in (1, 2):
        board = ((((xs // period) + (ys // period)) & 1) * 255).astype(np.uint8)
        yield "checker%d" % period, np.repeat(board[:, :, None], c, axis=2).copy()
    ramp = ((xs * 255) // max(w - 1, 1)).astype(np.uint8)
    yield "ramp", np.stack([np.roll(ramp, k, axis=1) for k in range(c)], axis=2).copy()


@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("h", HEIGHTS)
def test_one_halving_equals_oracle_and_host(hip, oracle, w, h):
    from smvs_amd import device, host
    for c in (1, 2, 3, 4):
        for name, a in _contents(w, h, c):
            got = device.rescale_half_gaussian(a, 1)
            want = oracle.rescale_half_size_gaussian(a).reshape(got.shape)
            assert got.shape == ((h + 1) // 2, (w + 1) // 2, c)
            assert np.array_equal(got, want), (name, c)
            assert np.array_equal(got, host.rescale_half_size_gaussian(a)), (name, c)
            # the host mirror's device function is the same call
            if name == "random":
                assert np.array_equal(host.rescale_half_size_gaussian(a, 1, device=0), want)


@pytest.mark.parametrize("w,h,c,halvings", [(515, 67, 3, 2), (515, 67, 3, 3), (5, 7, 1, 2),
                                            (5, 7, 1, 3), (4, 4, 3, 2)])
def test_chains_equal_the_oracle_applied_repeatedly(hip, oracle, w, h, c, halvings):
    """the levels ping-pong on the device; 5 x 7 passes through a 2-wide level
    (3 x 4, 2 x 2, 1 x 1), 4 x 4 ends at 1 x 1"""
    from smvs_amd import device, host
    rng = np.random.default_rng(w * h + halvings)
    a = rng.integers(0, 256, (h, w, c)).astype(np.uint8)
    want = a
    for _ in range(halvings):
        want = oracle.rescale_half_size_gaussian(want).reshape(
            (want.shape[0] + 1) // 2, (want.shape[1] + 1) // 2, c)
    got = device.rescale_half_gaussian(a, halvings)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert np.array_equal(host.rescale_half_size_gaussian(a, halvings, device=0), want)


def test_scene_option_gives_the_host_paths_files(hip, tmp_path):
    """reconstruct_scene(device_input_scaling=True) on the scene of
    test_reconstruct_scene_makescene_directory_with_automatic_input_scale:
    the undist-L1 images and the result embeddings of the run with the host
    loop, byte for byte."""
    from smvs_amd import synth, host, mve_scene
    inputs = synth.pipeline_inputs("sphere", 768, 512, 3, flen=1.2)
    dirs = {}
    for flag in (False, True):
        d = str(tmp_path / ("device" if flag else "host"))
        os.makedirs(d)
        mve_scene.write_scene(d, inputs, container="png")
        done, skipped, secs, scale = host.reconstruct_scene(
            d, view_ids=[0], num_neighbors=3, min_neighbors=2, output_scale=2, input_scale=-1,
            max_pixels=150000, details=True, device_input_scaling=flag)
        assert scale == 1 and done == [0] and skipped == 0
        dirs[flag] = d
    views = sorted(os.listdir(os.path.join(dirs[False], "views")))
    assert views == sorted(os.listdir(os.path.join(dirs[True], "views")))
    scaled = 0
    for v in views:
        a, b = (os.path.join(dirs[f], "views", v, "undist-L1.png") for f in (False, True))
        assert os.path.exists(a) == os.path.exists(b), v
        if os.path.exists(a):
            ia, ib = host.load_byte_image(a), host.load_byte_image(b)
            assert ia.shape == (256, 384, 3) and np.array_equal(ia, ib), v
            scaled += 1
    assert scaled >= 3   # the reference view and its neighbours
    for name in ("smvs-B1.mvei", "smvs-B1N.mvei"):
        fa, fb = (os.path.join(dirs[f], "views", "view_0000.mve", name) for f in (False, True))
        with open(fa, "rb") as f:
            da = f.read()
        with open(fb, "rb") as f:
            db = f.read()
        assert len(da) > 1000 and da == db, name
