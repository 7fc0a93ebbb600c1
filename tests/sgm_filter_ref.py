"""numpy restatement of the two filters of the SGM front end (include/smvs_hip.h,
"Two single-run rejections"): the uniqueness test on the
aggregated sums and the speckle removal on a depth map.

The uniqueness test is integers only.  The speckle filter's one float operation
is an np.float32 division of np.float32 values (IEEE, nothing to contract); its
components come from a plain union-find over the link edges."""
import numpy as np

F = np.float32


# ------------------------------------------------------------------ uniqueness
def uniqueness(S, argmin, uniq, window):
    """-> (rejected (h, w) bool, runner_up (h, w) u16, none (h, w) bool) for the
    volume S (h, w, D) of u16 sums and its winners: the competitors of winner i
    are the planes d with |d - i| > window, r their smallest sum; none: no
    competitor (runner_up 65535, never rejected); rejected iff
    r * (100 - uniq) < S[i] * 100."""
    S = np.asarray(S).astype(np.int64)
    h, w, D = S.shape
    i = np.asarray(argmin).astype(np.int64)
    d = np.arange(D, dtype=np.int64)[None, None, :]
    comp = np.abs(d - i[:, :, None]) > int(window)
    none = ~comp.any(axis=2)
    r = np.where(comp, S, np.int64(1) << 40).min(axis=2)
    b = np.take_along_axis(S, i[:, :, None], axis=2)[:, :, 0]
    rejected = ~none & (r * (100 - int(uniq)) < b * 100)
    runner_up = np.where(none, 65535, r).astype(np.uint16)
    return rejected, runner_up, none


def runner_up_plane(S, argmin, window):
    """the first plane that holds the runner-up's sum among the competitors, -1
    without one (for the counts of the tests: where the runner-up sits)"""
    S = np.asarray(S).astype(np.int64)
    D = S.shape[2]
    i = np.asarray(argmin).astype(np.int64)
    d = np.arange(D, dtype=np.int64)[None, None, :]
    comp = np.abs(d - i[:, :, None]) > int(window)
    pos = np.where(comp, S, np.int64(1) << 40).argmin(axis=2)
    return np.where(comp.any(axis=2), pos, -1)


def apply_uniqueness(depth, rejected):
    """a rejected pixel gets depth 0, every other pixel keeps its bits"""
    return np.where(rejected, F(0), np.asarray(depth, F)).astype(F)


# --------------------------------------------------------------------- speckles
def _links(depth, ratio):
    """-> (right (h, w - 1) bool, down (h - 1, w) bool): pixel linked with its
    neighbour at x + 1 / y + 1"""
    a = np.asarray(depth, F)
    valid = a > F(0)            # a NaN is not
    ratio = F(ratio)

    def linked(p, q, vp, vq):
        with np.errstate(invalid="ignore", divide="ignore"):
            quotient = (np.fmin(p, q) / np.fmax(p, q)).astype(F)
            return vp & vq & (quotient >= ratio)
    return (linked(a[:, :-1], a[:, 1:], valid[:, :-1], valid[:, 1:]),
            linked(a[:-1, :], a[1:, :], valid[:-1, :], valid[1:, :]))


def component_sizes(depth, ratio):
    """size (h, w) u32: the pixel count of every valid pixel's component under
    the links, 0 for a pixel that is not valid.  Union-find, smaller index as the
    root, path halving."""
    a = np.asarray(depth, F)
    h, w = a.shape
    right, down = _links(a, ratio)
    idx = np.arange(h * w, dtype=np.int64).reshape(h, w)
    pairs = np.concatenate([np.stack([idx[:, :-1][right], idx[:, 1:][right]], axis=1),
                            np.stack([idx[:-1, :][down], idx[1:, :][down]], axis=1)])
    parent = list(range(h * w))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for p, q in pairs.tolist():
        rp, rq = find(p), find(q)
        if rp < rq:
            parent[rq] = rp
        elif rq < rp:
            parent[rp] = rq
    roots = np.array([find(x) for x in range(h * w)], dtype=np.int64)
    valid = (a > F(0)).ravel()
    counts = np.bincount(roots[valid], minlength=h * w)
    size = np.where(valid, counts[roots], 0)
    return size.astype(np.uint32).reshape(h, w)


def filter_speckles(depth, speckle_size, ratio):
    """-> (out, size): out is 0 where 0 < size < speckle_size and the input's
    bits everywhere else (a NaN, a negative and a zero keep theirs)."""
    a = np.ascontiguousarray(depth, F)
    size = component_sizes(a, ratio)
    out = a.copy()
    out[(size > 0) & (size < int(speckle_size))] = F(0)
    return out, size
