"""The inputs and boxes that tests/test_tsdf_cull_cpu.py and tests/
test_gpu_tsdf_cull.py share: the sphere views of tests/test_gpu_tsdf_sparse.py
(1 % holes, noise, a depth step in view 0) and the boxes of its cases."""
import numpy as np

VOXEL = 0.06
SMALL = ((-1.1, -0.9, 2.8), VOXEL, (37, 29, 23))
DEEP = ((-1.22, -1.06, 0.45), 0.04, (61, 53, 75))
FREE = ((-0.3, -0.2, 1.0), 0.03, (9, 8, 7))
HALF_OUTSIDE = ((-1.0, -0.2, 2.8), VOXEL, (37, 29, 23))
AROUND_CAMERA = ((-0.6, -0.5, -0.62), 0.15, (8, 7, 41))
# as AROUND_CAMERA, the first slab of bricks across z = 0 of the camera at the origin
STRADDLE = ((-0.6, -0.5, -0.32), 0.15, (8, 7, 41))
BAR =((-1.2, -0.005, 3.1), 0.0006, (4096, 16, 12))
FINE = ((-1.3, -1.1, 0.4), 0.016, (160, 144, 200))
TWO_CUBED = ((-0.06, -0.06, 2.95), VOXEL, (2, 2, 2))
HUGE = ((-4.1, -4.1, 2.499), 0.002, (4096, 4096, 264))
HUGE_WINDOW = ((1920, 1952, 232), (2176, 2144, 264))


def inputs(n_views, w=97, h=63, channels=3, seed=5, last_size=None, shift=None, roll=None):
    """cams, depths, normals, images.  last_size: the last view has a size of
    its own; shift: the whole world (the cameras) moved by it; roll: the last
    camera turned about its axis by that angle."""
    from smvs_amd import synth
    base = synth.pipeline_inputs("sphere", w, h, max(n_views - 1, 1), flen=1.2)
    cams = base["cams"][:n_views]
    if last_size is not None:
        c = cams[-1]
        cams[-1] = synth.Camera(c.R, c.t, c.flen, last_size[0], last_size[1])
    if roll is not None:
        c = cams[-1]
        cs, sn = np.cos(roll), np.sin(roll)
        Rz = np.array([[cs, -sn, 0.0], [sn, cs, 0.0], [0.0, 0.0, 1.0]])
        cams[-1] = synth.Camera(Rz @ c.R, Rz @ c.t, c.flen, c.width, c.height)
    depths, normals = synth.depth_and_normal_maps(base["scene"], cams)
    rng = np.random.default_rng(seed)
    images = []
    for i in range(n_views):
        depths[i] *= (1.0 + 0.002 * rng.standard_normal(depths[i].shape)).astype(np.float32)
        depths[i][rng.random(depths[i].shape) < 0.01] = 0.0          # holes
    depths[0][h // 5:h // 5 + 9, w // 4:w // 4 + 13] *= np.float32(0.8)   # a step
    for d in depths:
        images.append(rng.integers(0, 256, d.shape if channels == 1 else d.shape + (channels,))
                      .astype(np.uint8))
    if shift is not None:
        s = np.asarray(shift, float)
        cams = [synth.Camera(c.R, c.t - c.R @ s, c.flen, c.width, c.height) for c in cams]
    return cams, depths, normals, images


def huge_inputs():
    """the one narrow 32 x 24 view of the 4096 x 4096 x 264 case"""
    from smvs_amd import synth
    cam = synth.Camera(np.eye(3), np.zeros(3), 8.0, 32, 24)
    depths, normals = synth.depth_and_normal_maps(synth.SphereScene(), [cam])
    rng = np.random.default_rng(3)
    images = [rng.integers(0, 256, (24, 32, 3)).astype(np.uint8)]
    depths[0][5, 7] = 0.0
    return [cam], depths, normals, images
