"""Case builders for the mesh clean (smvs_mesh_clean), shared by the CPU tests
of the restatement and the GPU tests of the device.  Every case scatters its
vertex ids with a seeded permutation, so that component roots do not sit at
block starts.  A case is (name, mesh dict, options dict); the mesh carries
`cells` (the tests drop it for the runs without)."""
import functools

import numpy as np

import mesh_clean_ref as ref

CS = 12              # component_size of the group cases
LOW, CUT = 0.05, 0.1  # a low confidence and the threshold that cuts it
GROUP_N = (1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 70001)


def make_mesh(n, faces, seed, conf=None):
    rng = np.random.default_rng(seed)
    xyz = rng.standard_normal((n, 3)).astype(np.float32)
    nrm = rng.standard_normal((n, 3)).astype(np.float32)
    rgb = rng.integers(0, 256, (n, 3), dtype=np.uint8)
    if conf is None:
        conf = rng.uniform(0.2, 1.0, n)
    cells = rng.permutation(4 * n + 7)[:n].astype(np.int64) * 3
    return {"xyz": xyz, "normals": nrm, "rgb": rgb,
            "confidence": np.ascontiguousarray(conf, np.float32),
            "faces": np.ascontiguousarray(faces, np.uint32).reshape(-1, 3), "cells": cells}


# The groups every case with n >= 63 starts with (63 vertices): 1, CS - 1 and a
# group of two are removed as small; CS, CS + 1 and CS are kept, the first at
# exactly component_size; the last CS has one vertex cut and falls apart into
# small pieces.  No chance is involved, so the wave-edge sizes carry them too.
FIXED_SIZES = (1, CS - 1, 2, CS, CS + 1, CS, CS)
CUT_GROUP = 6        # index in FIXED_SIZES of the group that gets a cut vertex


def group_sizes(n, rng):
    """FIXED_SIZES first (as far as n has room), a 300 where it fits, then sizes
    from 1 .. 300, small and large in turn"""
    sizes, left = [], n
    for s in FIXED_SIZES + (300,):
        if s <= left:
            sizes.append(s)
            left -= s
        elif s != 300:
            break
    turn = 0
    while left > 0:
        hi = min(300, left)
        if turn % 2 == 0 or hi < CS:
            s = int(rng.integers(1, min(CS - 1, hi) + 1))
        else:
            s = int(rng.integers(CS, hi + 1))
        sizes.append(s)
        left -= s
        turn += 1
    return sizes


def groups(n, seed, dense):
    """n vertices in groups; inside a group a triangle strip (it makes the group
    one component) and, with dense, 2 g random triangles on top (m > n; without,
    m < n).  A group of two has one face with a repeated id.  Group CUT_GROUP
    and, behind the fixed groups, every third group of 5 or more have one
    low-confidence vertex in their strip: the cut splits them."""
    rng = np.random.default_rng(seed)
    sizes = group_sizes(n, rng)
    perm = rng.permutation(n)
    conf = rng.uniform(0.2, 1.0, n)
    fixed = len(FIXED_SIZES)
    faces, start = [], 0
    for gi, g in enumerate(sizes):
        ids = perm[start:start + g]
        if g == 2:
            faces.append(np.array([[ids[0], ids[1], ids[1]]]))
        elif g >= 3:
            i = np.arange(g - 2)
            faces.append(np.stack([ids[i], ids[i + 1], ids[i + 2]], 1))
            if dense:
                faces.append(ids[rng.integers(0, g, (2 * g, 3))])   # (some repeat an id)
            if sizes[:fixed] == list(FIXED_SIZES) and gi == CUT_GROUP:
                conf[ids[g // 2]] = LOW
            elif gi > fixed and gi % 3 == 0 and g >= 5:
                conf[ids[int(rng.integers(1, g - 1))]] = LOW
        start += g
    fc = np.concatenate(faces) if faces else np.zeros((0, 3), np.int64)
    fc = fc[rng.permutation(fc.shape[0])]
    return make_mesh(n, fc, seed + 1, conf), sizes


def strip(n, order, seed=5):
    """one triangle strip: deep chains towards the low ids"""
    rng = np.random.default_rng(seed)
    ids = rng.permutation(n) if order == "permuted" else np.arange(n)[::-1]
    i = np.arange(n - 2)
    return make_mesh(n, np.stack([ids[i], ids[i + 1], ids[i + 2]], 1), seed + 1)


def fan(n, seed=9):
    """one hub vertex in every face: contention on one label"""
    rng = np.random.default_rng(seed)
    ids = rng.permutation(n)
    i = np.arange(1, n - 1)
    return make_mesh(n, np.stack([np.full(n - 2, ids[0]), ids[i], ids[i + 1]], 1), seed + 1)


BRIDGE_A, BRIDGE_B = 40, 15


def bridge(seed=13):
    """two strips of 40 and 15 vertices joined only by faces through one
    low-confidence vertex: the cut splits them, the 15 fall below 20"""
    rng = np.random.default_rng(seed)
    n = BRIDGE_A + BRIDGE_B + 1
    ids = rng.permutation(n)
    a, b, j = ids[:BRIDGE_A], ids[BRIDGE_A:BRIDGE_A + BRIDGE_B], ids[-1]
    fa = np.stack([a[:-2], a[1:-1], a[2:]], 1)
    fb = np.stack([b[:-2], b[1:-1], b[2:]], 1)
    joint = np.array([[a[-1], j, b[0]], [a[-2], a[-1], j], [j, b[0], b[1]]])
    conf = rng.uniform(0.6, 1.0, n)
    conf[j] = LOW
    return make_mesh(n, np.concatenate([fa, joint, fb]), seed + 1, conf), a, b, j


def small_mesh():
    """written by hand (tests/test_mesh_clean_cpu.py has the answers): a
    triangle pair 0-1-2-3, a face with a repeated id on 4 and 5, the isolated
    vertex 6, a triangle 7-8-9 whose vertex 8 is cut"""
    faces = [[0, 1, 2], [2, 1, 3], [4, 5, 5], [7, 8, 9]]
    conf = [0.9, 0.8, 0.7, 0.6, 0.5, 0.5, 0.9, 0.4, 0.01, 0.3]
    return make_mesh(10, faces, 21, conf)


def ties(n, seed=17, nan=True):
    """confidences from {j / 16} in long runs over a strip, one NaN (with nan)
    and one -0.0 among them (n >= 8)"""
    rng = np.random.default_rng(seed)
    conf = (np.sort(rng.integers(0, 5, n)) / 16.0).astype(np.float32)
    if n >= 8:
        if nan:
            conf[-1] = np.nan
        conf[0] = -0.0
    conf = conf[rng.permutation(n)]
    i = np.arange(max(n - 2, 0))
    ids = rng.permutation(n)
    return make_mesh(n, np.stack([ids[i], ids[i + 1], ids[i + 2]], 1), seed + 1, conf)


def tie_percentiles(conf):
    """percentiles that put k on the first element, inside and on the last
    element of the longest run of equal confidences (in key order), and 100"""
    n = conf.size
    key = np.sort(ref.float_key(conf))
    starts = np.flatnonzero(np.r_[True, key[1:] != key[:-1]])
    ends = np.r_[starts[1:], n] - 1
    r = int(np.argmax(ends - starts))
    out = []
    for k in (starts[r], (starts[r] + ends[r]) // 2, ends[r]):
        # the smallest float32 percentile whose k is this one
        p = np.float32(100.0 * k / (n - 1)) if k else np.float32(1e-3)   # (0 is "off")
        while int(float(p) * float(n - 1) / 100.0) < k:
            p = np.nextafter(p, np.float32(200))
        if 0 < p <= 100 and int(float(p) * float(n - 1) / 100.0) == k:
            out.append((int(k), float(p)))
    out.append((n - 1, 100.0))
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = []
    for n in GROUP_N:
        for dense in (False, True):
            mesh, _sizes = groups(n, 100 + n, dense)
            cases.append(("groups-%d-%s" % (n, "dense" if dense else "sparse"), mesh,
                          dict(threshold=CUT, component_size=CS)))
    for order in ("permuted", "reversed"):
        cases.append(("strip-" + order, strip(5000, order), dict(component_size=1000)))
    cases.append(("fan", fan(3000), dict(component_size=1000)))
    cases.append(("bridge", bridge()[0], dict(threshold=0.5, component_size=20)))
    for keep in (False, True):
        cases.append(("small-keep%d" % keep, small_mesh(),
                      dict(threshold=CUT, component_size=4, keep_unreferenced=keep)))
        cases.append(("small-nocomp-keep%d" % keep, small_mesh(),
                      dict(threshold=CUT, component_size=1, keep_unreferenced=keep)))
    mesh = ties(96)
    for k, p in tie_percentiles(mesh["confidence"]):
        cases.append(("ties-k%d" % k, mesh, dict(percentile=p, component_size=1)))
    cases.append(("ties-p10-comp", mesh, dict(percentile=10.0, component_size=8)))
    # without the NaN percentile 100 gives t = the maximum: nothing equal to it is cut
    cases.append(("ties-max-p100", ties(96, nan=False), dict(percentile=100.0, component_size=1)))
    for n in (1, 2):
        mesh = ties(n)
        for p in (50.0, 100.0):
            cases.append(("ties-n%d-p%d" % (n, p), mesh,
                          dict(percentile=p, component_size=1, keep_unreferenced=True)))
    big, _sizes = groups(70001, 7, True)
    cases.append(("groups-70001-p10", big, dict(percentile=10.0, component_size=CS)))
    empty = make_mesh(0, np.zeros((0, 3)), 1)
    cases.append(("empty-n0", empty, dict(threshold=CUT, component_size=CS)))
    cases.append(("empty-n0-p10", empty, dict(percentile=10.0, component_size=CS)))
    cases.append(("empty-m0", make_mesh(300, np.zeros((0, 3)), 2),
                  dict(component_size=1, keep_unreferenced=True)))
    cases.append(("empty-m0-drop", make_mesh(300, np.zeros((0, 3)), 2), dict(component_size=1)))
    cases.append(("all-cut", groups(257, 3, True)[0], dict(threshold=2.0, component_size=CS)))
    return tuple(cases)


def case_names():
    return [c[0] for c in all_cases()]


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (mesh, options, the restatement's result with cells); computed once,
    shared, and not to be changed by a test"""
    for nm, mesh, opts in all_cases():
        if nm == name:
            return mesh, opts, ref.clean(mesh, **opts)
    raise KeyError(name)


def tally(name):
    """what a case exercises, from the restatement's result"""
    mesh, opts, out = case(name)
    cs = opts.get("component_size", 1000)
    comp, size = out["component"], out["component_size"]
    roots = comp == np.arange(comp.size)
    faces = mesh["faces"].astype(np.int64)
    cut = comp == ref.NO_COMPONENT
    repeated = (faces[:, 0] == faces[:, 1]) | (faces[:, 1] == faces[:, 2]) \
        | (faces[:, 0] == faces[:, 2]) if faces.size else np.zeros(0, bool)
    by_cut = cut[faces].any(1) if faces.size else np.zeros(0, bool)
    return {"n": comp.size, "m": faces.shape[0],
            "small_removed": int((roots & (size < cs)).sum()) if cs > 1 else 0,
            "kept": int((roots & (out["new_id"] >= 0)).sum()),
            "kept_at_size": int((roots & (size == cs) & (out["new_id"] >= 0)).sum()),
            "cut": int(cut.sum()), "faces_cut": int(by_cut.sum()),
            "faces_repeated": int((repeated & ~by_cut).sum()),
            "out_n": out["confidence"].size, "out_m": out["faces"].shape[0]}
