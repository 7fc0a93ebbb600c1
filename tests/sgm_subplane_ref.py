"""numpy restatement of the sub-plane winner of the SGM front end
(SMVS_SGM_WINNER_SUBPLANE, include/smvs_hip.h).

Every float operation is one np.float32 operation in the written order: numpy
rounds each to float, so there is nothing to contract and the division is
IEEE's."""
import numpy as np

F = np.float32


def inv_table(min_depth, max_depth, D):
    """inv[k], the inverse depth of plane k as lib/sgm_stereo.cc:197-203
    accumulates it in float: the planes' depths are 1.0f / inv[k]."""
    inv = np.zeros(D, F)
    v = F(1.0) / F(max_depth)
    inc = (F(1.0) / F(min_depth) - v) / F(D - 1)
    for k in range(D):
        inv[k] = v
        v = F(v + inc)
    return inv


def winner_offsets(S, argmin):
    """-> (off, den, neighbour plane n) of every pixel for the volume S
    (h, w, D) and its winners; off == 0 and n == i - 1 where the definition
    gives no offset (last plane, den == 0).  Pixels with i < 1 get a, den of a
    clamped index: they are invalid anyway (i < 2)."""
    S = np.asarray(S).astype(np.int64)
    D = S.shape[2]
    i = np.asarray(argmin).astype(np.int64)
    pick = lambda k: np.take_along_axis(S, np.clip(k, 0, D - 1)[:, :, None], axis=2)[:, :, 0]
    a, b, c = pick(i - 1), pick(i), pick(i + 1)
    den = a - 2 * b + c
    none = (i == D - 1) | (den == 0)
    num = (a - c).astype(F)
    safe = np.where(none, 1, 2 * den).astype(F)
    off = np.where(none, F(0), num / safe).astype(F)
    n = np.where(off > 0, i + 1, i - 1)
    return off, np.where(i == D - 1, 0, den), n


def subplane_depth(S, argmin, main_img, min_depth, max_depth):
    """The depth map of the definition: 0 for i < 2 or main_img < 25 (the rule
    of lib/sgm_stereo.cc:300-303), else 1 / (inv[i] + |off| (inv[n] - inv[i]))."""
    S = np.asarray(S)
    D = S.shape[2]
    inv = inv_table(min_depth, max_depth, D)
    i = np.asarray(argmin).astype(np.int64)
    off, _, n = winner_offsets(S, i)
    valid = (i >= 2) & (np.asarray(main_img) >= 25)
    base = inv[i]
    step = (np.abs(off) * (inv[np.clip(n, 0, D - 1)] - base).astype(F)).astype(F)
    r = (base + step).astype(F)
    with np.errstate(divide="ignore"):
        depth = (F(1.0) / r).astype(F)
    return np.where(valid, depth, F(0)).astype(F)


def scene_pair():
    """The pair of tests/test_gpu_sgm_subplane.py (and of the CPU counts beside
    it): views 0 and 1 of synth.pipeline_inputs("sphere", 192, 128, 2, flen=1.2)
    at SGM scale 1 (96 x 64) with the reprojection main -> neighbour.  Host
    code only."""
    from smvs_amd import host, synth
    inputs = synth.pipeline_inputs("sphere", 192, 128, 2, flen=1.2)
    imgs = [host.sgm_image(inputs, k, 1) for k in range(2)]
    M, t = host.view_reprojection(dict(inputs, images=imgs), 0, 1)
    return imgs[0], imgs[1], M, t
