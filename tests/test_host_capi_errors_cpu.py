"""The argument checks of the host C ABI (csrc/host/host_capi.h), pinned: a
table of calls into libsmvs_host.so that each fail on an argument check before
any device call and before any file is opened, with the status and the exact
smvs_host_last_error() text recorded in tests/golden/host_capi_errors.json.

The texts name the entry that introduced the check, which is often not the one
called (a bad filter met through smvs_host_reconstruct_scene_refine is reported
as ..._scene_filtered); cases that violate two checks at once pin the order of
the checks.  Both are part of the contract.

`python tests/test_host_capi_errors_cpu.py --record` rewrites the JSON from the
library as built; it was recorded before the ABI's source was split."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "host_capi_errors.json")

_fp = C.POINTER(C.c_float)
_u8p = C.POINTER(C.c_uint8)
_i32p = C.POINTER(C.c_int32)
f32 = C.c_float
NAN = float("nan")


def _host():
    from smvs_amd import host
    host.load()
    return host


# ---------------------------------------------------------------- arguments
# (every buffer a case hands over is real and large enough: a case fails on its
# check, not on the memory behind a pointer)
_W, _H = 8, 6
_IMG = np.full((_H, _W, 1), 90, np.uint8)
_DEPTH = np.full((_H, _W), 5.0, np.float32)
_SLANT = np.zeros((_H, _W, 2), np.float32)
_FEATS = np.array([[0.0, 0.0, 5.0]], np.float32)
_OFFS = np.array([0, 2], np.int32)
_REFS = np.array([0, 1], np.int32)
_INFO = np.zeros(6, np.int32)
_NODES = np.zeros((_W + 2) * (_H + 2) * 4)
_NV = np.zeros((_W + 2) * (_H + 2), np.uint8)
_PV = np.zeros((_W + 1) * (_H + 1), np.uint8)
_OPS_UNKNOWN = np.array([9, 0], np.int32)
_OPS_NONE = np.zeros(1, np.int32)
_OUT_F = np.zeros(_W * _H * 3, np.float32)
_OUT_B = np.zeros(_W * _H * 4, np.uint8)
_OUT_I = np.zeros(16, np.int32)
_OUT_D = np.zeros(64)
_IDS = np.array([0], np.int32)
_NOWHERE = b"/no/such/scene"

fptr = lambda a: a.ctypes.data_as(_fp)
bptr = lambda a: a.ctypes.data_as(_u8p)
iptr = lambda a: a.ctypes.data_as(_i32p)
dptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))


def _view(host, view_id, tx):
    v = host.HostView()
    v.width, v.height, v.channels = _W, _H, 1
    v.bytes = bptr(_IMG)
    v.flen = 1.0
    for i in range(9):
        v.rot[i] = float(i % 4 == 0)
    v.trans[0] = tx
    v.view_id = view_id
    return v


class _Args:
    """What the cases share, made once."""

    def __init__(self):
        host = _host()
        self.host = host
        self.lib = host.load()
        self.main = _view(host, 0, 0.0)
        self.subs = (host.HostView * 3)(_view(host, 1, -0.1), _view(host, 2, 0.1),
                                        _view(host, 3, 0.2))
        self.bundle = host.HostBundle(1, fptr(_FEATS), iptr(_OFFS), iptr(_REFS))
        self.opts = host.HostOptions(0.01, 0.0, 5, 2, 0, 0, 0, 0, 0, 0)
        self.recon = host.ReconSettings(b"undistorted", 1.0, 2, 0, 1, 0, 0, 0, 0.0, 0.0, 1, 6,
                                        3, 0, 1, 2, -1, 1700000)
        self.pc = host.PointCloudSettings()
        self.pc.image_embedding = b"undistorted"
        self.fused = host.FusedSettings(0.0, 64, 0.0, 0)
        self.fused_sparse = host.FusedSparseSettings(0.0, 64, 0.0, 0, 0)
        self.fused_cull = host.FusedSparseCullSettings(0.0, 64, 0.0, 0, 0, 1)
        self.imp = host.ImportSettings()
        self.rep = host.ImportReport()


_ARGS = None


def _args():
    global _ARGS
    if _ARGS is None:
        _ARGS = _Args()
    return _ARGS


def sweep(on=1, min_views=-1, best_k=-1, support_cost=20, min_support=-1):
    return _args().host.SgmSweep(on, min_views, best_k, support_cost, min_support)


def filt(uniqueness=0, window=1, speckle_size=0, speckle_ratio=0.95):
    return _args().host.SgmFilter(uniqueness, window, speckle_size, speckle_ratio)


def photo(radius=0, best_k=2, min_views=2, min_score=0.49, witnesses=-1):
    return _args().host.SgmPhoto(radius, best_k, min_views, min_score, witnesses)


def refine(sweeps=0, samples=2, depth_step=0.02, slant_step=0.01, seed=1, fill=1):
    return _args().host.SgmRefine(sweeps, samples, depth_step, slant_step, seed, fill)


def _ref(x):
    return None if x is None else C.byref(x)


# ------------------------------------------------------------ sgm_depth family
def sgm_depth(entry, n_subs=2, num_steps=128, subplane=0, neighbors=2, consensus=0,
              agree_ratio=0.95, min_agree=2, sw=None, fl=None, ph=None, rf=None):
    """One call of smvs_host_sgm_depth<entry> with the arguments that entry takes
    (the main view and its neighbours are valid: the newest entry reads them)."""
    a = _args()
    head = (C.byref(a.main), a.subs, C.c_int(n_subs), C.byref(a.bundle), C.c_int(1), f32(1.0),
            f32(8.0), C.c_int(0))
    tail = (fptr(_OUT_F), iptr(_OUT_I), iptr(_OUT_I[1:]))
    merge = (C.c_int(neighbors), C.c_int(consensus), f32(agree_ratio), C.c_int(min_agree))
    mid = {
        "": (),
        "_mode": (C.c_int(0),),
        "_steps": (C.c_int(0), C.c_int(num_steps)),
        "_subplane": (C.c_int(0), C.c_int(num_steps), C.c_int(subplane)),
        "_merge": (C.c_int(0), C.c_int(num_steps), C.c_int(subplane)) + merge,
        "_sweep": (C.c_int(0), C.c_int(num_steps), C.c_int(subplane)) + merge + (_ref(sw),),
        "_filtered": (C.c_int(0), C.c_int(num_steps), C.c_int(subplane)) + merge
        + (_ref(sw), _ref(fl)),
    }
    fn = getattr(a.lib, "smvs_host_sgm_depth" + entry)
    if entry == "_photo":
        return fn(*head, C.c_int(0), C.c_int(num_steps), C.c_int(subplane), *merge, _ref(sw),
                  _ref(fl), _ref(ph), fptr(_OUT_F), fptr(_OUT_F), iptr(_OUT_I), iptr(_OUT_I[1:]))
    if entry == "_refine":
        return fn(*head, C.c_int(0), C.c_int(num_steps), C.c_int(subplane), *merge, _ref(sw),
                  _ref(fl), _ref(ph), _ref(rf), fptr(_OUT_F), fptr(_OUT_F), fptr(_OUT_F),
                  iptr(_OUT_I), iptr(_OUT_I[1:]))
    return fn(*head, *mid[entry], *tail)


# ---------------------------------------------------------------- scene family
def scene(entry, scene_dir=_NOWHERE, settings=True, flags=0, num_steps=128, subplane=0,
          neighbors=2, consensus=0, agree_ratio=0.95, min_agree=2, sw=None, fl=None, ph=None,
          rf=None):
    """One call of smvs_host_reconstruct_scene<entry> with the arguments that
    entry takes; the scene directory does not exist and is never opened."""
    a = _args()
    head = (scene_dir, C.byref(a.recon) if settings else None)
    tail = (None, C.c_int(0), iptr(_OUT_I), C.c_int(4), iptr(_OUT_I[4:]), iptr(_OUT_I[5:]),
            dptr(_OUT_D), iptr(_OUT_I[6:]))
    steps = (C.c_uint(flags), C.c_int(num_steps))
    merge = steps + (C.c_int(subplane), C.c_int(neighbors), C.c_int(consensus),
                     f32(agree_ratio), C.c_int(min_agree))
    mid = {
        "": (),
        "_mode": (C.c_int(flags),),
        "_flags": (C.c_uint(flags),),
        "_steps": steps,
        "_subplane": steps + (C.c_int(subplane),),
        "_merge": merge,
        "_sweep": merge + (_ref(sw),),
        "_filtered": merge + (_ref(sw), _ref(fl)),
        "_photo": merge + (_ref(sw), _ref(fl), _ref(ph)),
        "_refine": merge + (_ref(sw), _ref(fl), _ref(ph), _ref(rf)),
        "_planes": merge + (_ref(sw), _ref(fl), _ref(ph), _ref(rf)),
    }
    return getattr(a.lib, "smvs_host_reconstruct_scene" + entry)(*head, *mid[entry], *tail)


SCENE_ENTRIES = ("", "_mode", "_flags", "_steps", "_subplane", "_merge", "_sweep", "_filtered",
                 "_photo", "_refine", "_planes")
# the entries that take a flags word, bit 32 refused by all but _planes
SCENE_FLAG_ENTRIES = SCENE_ENTRIES[2:]


def optimize_planes(flags, slant, sw_, sh_, sc_):
    a = _args()
    return a.lib.smvs_host_optimize_planes(
        C.byref(a.main), a.subs, C.c_int(2), C.byref(a.bundle), None, C.c_int(0), C.c_int(0),
        None, fptr(_SLANT) if slant else None, C.c_int(sw_), C.c_int(sh_), C.c_int(sc_),
        C.byref(a.opts), C.c_uint(flags), None, None, None)


def optimize_flags(flags):
    a = _args()
    return a.lib.smvs_host_optimize_flags(
        C.byref(a.main), a.subs, C.c_int(2), C.byref(a.bundle), None, C.c_int(0), C.c_int(0),
        None, C.byref(a.opts), C.c_uint(flags), None, None, None)


def surface_script(entry, main=True, depth=True, slant=True, ops=_OPS_NONE, n_ops=0,
                   delete_every=3, info=True):
    a = _args()
    m = C.byref(a.main) if main else None
    d = fptr(_DEPTH) if depth else None
    s = fptr(_SLANT) if slant else None
    tail = (iptr(_INFO) if info else None, dptr(_NODES), bptr(_NV), bptr(_PV))
    script = (C.c_int(2), iptr(ops), C.c_int(n_ops), C.c_int(delete_every))
    fn = getattr(a.lib, "smvs_host_surface_script" + entry)
    if entry == "":
        return fn(m, C.byref(a.bundle), d, *script, *tail)
    if entry == "_device":
        return fn(m, C.byref(a.bundle), d, *script, C.c_int(0), *tail)
    if entry == "_planes":
        return fn(m, d, s, *script, *tail)
    return fn(m, d, s, *script, C.c_int(0), *tail)


def surface_maps(entry, n_subs=2, depth=True, slant=True, out=True):
    a = _args()
    d = fptr(_DEPTH) if depth else None
    s = fptr(_SLANT) if slant else None
    o = fptr(_OUT_F) if out else None
    if entry == "_host":
        return a.lib.smvs_host_surface_maps_host(C.byref(a.main) if out else None, d, s,
                                                 C.c_int(2), fptr(_OUT_F), fptr(_OUT_F))
    if entry == "_planes":
        return a.lib.smvs_host_surface_maps_planes(C.byref(a.main), a.subs, C.c_int(n_subs),
                                                   C.byref(a.bundle), d, s, C.c_int(2),
                                                   C.c_int(0), o, o)
    return a.lib.smvs_host_surface_maps(C.byref(a.main), a.subs, C.c_int(n_subs),
                                        C.byref(a.bundle), d, C.c_int(2), C.c_int(0), o, o)


def export(entry, scene_dir=_NOWHERE, settings=True, fused=True, ids=True, n_ids=0):
    """smvs_host_generate<entry>: the point cloud, the two meshes, the three
    fused forms."""
    a = _args()
    path = C.create_string_buffer(64)
    n1, n2 = C.c_int64(0), C.c_int64(0)
    fn = getattr(a.lib, "smvs_host_generate" + entry)
    st = C.byref(a.pc) if settings else None
    idp = iptr(_IDS) if ids else None
    if entry == "_point_cloud":
        return fn(scene_dir, st, idp, C.c_int(n_ids), path, C.c_int(64), C.byref(n1))
    if entry in ("_mesh", "_simplified"):
        return fn(scene_dir, st, idp, C.c_int(n_ids), path, C.c_int(64), C.byref(n1),
                  C.byref(n2))
    fs = dict(_fused=a.fused, _fused_sparse=a.fused_sparse, _fused_sparse_cull=a.fused_cull)
    return fn(scene_dir, st, C.byref(fs[entry]) if fused else None, idp, C.c_int(n_ids), path,
              C.c_int(64), C.byref(n1), C.byref(n2))


EXPORTS = ("_point_cloud", "_mesh", "_simplified", "_fused", "_fused_sparse",
           "_fused_sparse_cull")


def _build_cases():
    L = lambda: _args().lib
    A = _args
    c = {}

    # ---- optimizer entries
    c["optimize_flags/bit1"] = lambda: optimize_flags(2)
    c["optimize_flags/bit2"] = lambda: optimize_flags(4)
    c["optimize_planes/bit2"] = lambda: optimize_planes(4, False, 0, 0, 0)
    c["optimize_planes/slant_w0"] = lambda: optimize_planes(0, True, 0, _H, 2)
    c["optimize_planes/slant_h0"] = lambda: optimize_planes(2, True, _W, 0, 2)
    c["optimize_planes/slant_c0"] = lambda: optimize_planes(3, True, _W, _H, 0)
    c["optimize_planes/bit2+slant_w0"] = lambda: optimize_planes(4, True, 0, _H, 2)
    c["shading_planes/null"] = lambda: L().smvs_host_shading_planes(
        None, C.c_int(_W), C.c_int(_H), C.c_int(1), C.c_int(0), fptr(_OUT_F), fptr(_OUT_F))
    c["shading_planes/width0"] = lambda: L().smvs_host_shading_planes(
        bptr(_IMG), C.c_int(0), C.c_int(_H), C.c_int(1), C.c_int(0), fptr(_OUT_F), fptr(_OUT_F))
    c["shading_planes/channels0"] = lambda: L().smvs_host_shading_planes(
        bptr(_IMG), C.c_int(_W), C.c_int(_H), C.c_int(0), C.c_int(0), fptr(_OUT_F), fptr(_OUT_F))
    c["gamma_inv_srgb_lut/null"] = lambda: L().smvs_host_gamma_inv_srgb_lut(None)
    c["optimize_views/null_mains"] = lambda: L().smvs_host_optimize_views(
        None, A().subs, C.c_int(1), C.c_int(2), C.byref(A().bundle), C.byref(A().opts),
        C.c_int(1), C.c_int(0), C.c_int(1), C.c_int(1), C.c_int(0), None, None, None, None, None)
    c["optimize_views/no_jobs"] = lambda: L().smvs_host_optimize_views(
        C.byref(A().main), A().subs, C.c_int(0), C.c_int(2), C.byref(A().bundle),
        C.byref(A().opts), C.c_int(1), C.c_int(0), C.c_int(1), C.c_int(1), C.c_int(0), None,
        None, None, None, None)
    c["optimize_views/no_workers"] = lambda: L().smvs_host_optimize_views(
        C.byref(A().main), A().subs, C.c_int(1), C.c_int(2), C.byref(A().bundle),
        C.byref(A().opts), C.c_int(1), C.c_int(0), C.c_int(1), C.c_int(0), C.c_int(0), None,
        None, None, None, None)
    c["gn_solve_step/null_main"] = lambda: L().smvs_host_gn_solve_step(
        None, A().subs, C.c_int(2), C.byref(A().bundle), C.c_int(2), C.c_double(0.01),
        C.c_int(0), *([None] * 11))
    c["gn_solve_step/no_subs"] = lambda: L().smvs_host_gn_solve_step(
        C.byref(A().main), A().subs, C.c_int(0), C.byref(A().bundle), C.c_int(2),
        C.c_double(0.01), C.c_int(0), *([None] * 11))
    c["view_queue_selftest/negative"] = lambda: L().smvs_host_view_queue_selftest(
        C.c_int(-1), C.c_int(1), C.c_int(1), C.c_int(-1), iptr(_OUT_I), iptr(_OUT_I))
    c["view_queue_selftest/null_hist"] = lambda: L().smvs_host_view_queue_selftest(
        C.c_int(1), C.c_int(1), C.c_int(1), C.c_int(-1), None, iptr(_OUT_I))
    c["block_multiply/no_nodes"] = lambda: L().smvs_host_block_multiply(
        C.c_int(0), C.c_int(1), dptr(_OUT_D), dptr(_OUT_D), dptr(_OUT_D))
    c["block_multiply/null_x"] = lambda: L().smvs_host_block_multiply(
        C.c_int(1), C.c_int(1), dptr(_OUT_D), None, dptr(_OUT_D))
    c["select_neighbors/null_views"] = lambda: L().smvs_host_select_neighbors(
        None, C.c_int(3), None, C.c_int(0), C.c_int(2), iptr(_OUT_I), iptr(_OUT_I[8:]))
    c["select_neighbors/view_out_of_range"] = lambda: L().smvs_host_select_neighbors(
        A().subs, C.c_int(3), None, C.c_int(3), C.c_int(2), iptr(_OUT_I), iptr(_OUT_I[8:]))
    c["select_neighbors/negative_count"] = lambda: L().smvs_host_select_neighbors(
        A().subs, C.c_int(3), None, C.c_int(0), C.c_int(-1), iptr(_OUT_I), iptr(_OUT_I[8:]))

    # ---- the defaults getters
    c["sgm_default_switches/null"] = lambda: L().smvs_host_sgm_default_switches(None)
    c["sgm_sweep_defaults/null"] = lambda: L().smvs_host_sgm_sweep_defaults(None)
    for name in ("merge", "filter", "refine", "photo"):
        fn = "smvs_host_sgm_%s_defaults" % name
        c["sgm_%s_defaults/null_ints" % name] = \
            lambda fn=fn: getattr(L(), fn)(None, fptr(_OUT_F))
        c["sgm_%s_defaults/null_floats" % name] = \
            lambda fn=fn: getattr(L(), fn)(iptr(_OUT_I), None)

    # ---- smvs_host_sgm_depth_*: every entry, every check, and pairs of checks
    c["sgm_depth/no_neighbour"] = lambda: sgm_depth("", n_subs=0)
    c["sgm_depth_mode/no_neighbour"] = lambda: sgm_depth("_mode", n_subs=0)
    c["sgm_depth_steps/steps1"] = lambda: sgm_depth("_steps", num_steps=1)
    c["sgm_depth_steps/steps257"] = lambda: sgm_depth("_steps", num_steps=257)
    c["sgm_depth_steps/no_neighbour"] = lambda: sgm_depth("_steps", n_subs=0)
    c["sgm_depth_subplane/steps129"] = lambda: sgm_depth("_subplane", num_steps=129, subplane=1)
    c["sgm_depth_merge/three_without_consensus"] = lambda: sgm_depth("_merge", neighbors=3)
    c["sgm_depth_merge/zero_neighbours"] = lambda: sgm_depth("_merge", neighbors=0)
    c["sgm_depth_merge/seventeen_neighbours"] = \
        lambda: sgm_depth("_merge", neighbors=17, consensus=1)
    c["sgm_depth_merge/three+steps132"] = \
        lambda: sgm_depth("_merge", neighbors=3, num_steps=132)
    c["sgm_depth_sweep/sweep+consensus"] = \
        lambda: sgm_depth("_sweep", consensus=1, sw=sweep())
    c["sgm_depth_sweep/sweep+consensus+steps0"] = \
        lambda: sgm_depth("_sweep", consensus=1, sw=sweep(), num_steps=0)
    c["sgm_depth_sweep/sweep+consensus+three"] = \
        lambda: sgm_depth("_sweep", consensus=1, neighbors=3, sw=sweep())
    c["sgm_depth_sweep/sweep_off_three"] = \
        lambda: sgm_depth("_sweep", neighbors=3, sw=sweep(on=0))
    c["sgm_depth_filtered/uniqueness100"] = \
        lambda: sgm_depth("_filtered", fl=filt(uniqueness=100))
    c["sgm_depth_filtered/window0"] = lambda: sgm_depth("_filtered", fl=filt(window=0))
    c["sgm_depth_filtered/speckle_negative"] = \
        lambda: sgm_depth("_filtered", fl=filt(speckle_size=-1))
    c["sgm_depth_filtered/ratio_nan"] = \
        lambda: sgm_depth("_filtered", fl=filt(speckle_ratio=NAN))
    c["sgm_depth_filtered/filter+steps1"] = \
        lambda: sgm_depth("_filtered", fl=filt(window=257), num_steps=1)
    c["sgm_depth_filtered/filter+sweep+consensus"] = \
        lambda: sgm_depth("_filtered", fl=filt(uniqueness=-1), consensus=1, sw=sweep())
    c["sgm_depth_photo/radius4"] = lambda: sgm_depth("_photo", ph=photo(radius=4))
    c["sgm_depth_photo/best_k17"] = lambda: sgm_depth("_photo", ph=photo(radius=1, best_k=17))
    c["sgm_depth_photo/score_nan"] = \
        lambda: sgm_depth("_photo", ph=photo(radius=1, min_score=NAN))
    c["sgm_depth_photo/witnesses-2"] = \
        lambda: sgm_depth("_photo", ph=photo(radius=1, witnesses=-2))
    c["sgm_depth_photo/filter+photo"] = \
        lambda: sgm_depth("_photo", fl=filt(uniqueness=100), ph=photo(radius=4))
    c["sgm_depth_photo/photo+three"] = \
        lambda: sgm_depth("_photo", ph=photo(min_views=-1), neighbors=3)
    c["sgm_depth_refine/sweeps9"] = lambda: sgm_depth("_refine", rf=refine(sweeps=9))
    c["sgm_depth_refine/samples-1"] = lambda: sgm_depth("_refine", rf=refine(samples=-1))
    c["sgm_depth_refine/step_nan"] = lambda: sgm_depth("_refine", rf=refine(depth_step=NAN))
    c["sgm_depth_refine/slant_step2"] = lambda: sgm_depth("_refine", rf=refine(slant_step=2.0))
    c["sgm_depth_refine/fill2"] = lambda: sgm_depth("_refine", rf=refine(fill=2))
    c["sgm_depth_refine/photo+refine"] = \
        lambda: sgm_depth("_refine", ph=photo(radius=-1), rf=refine(sweeps=9))
    c["sgm_depth_refine/filter+refine"] = \
        lambda: sgm_depth("_refine", fl=filt(speckle_ratio=1.5), rf=refine(fill=-1))
    c["sgm_depth_refine/refine+steps130"] = \
        lambda: sgm_depth("_refine", rf=refine(sweeps=-1), num_steps=130)
    c["sgm_depth_refine/steps130"] = lambda: sgm_depth("_refine", num_steps=130)
    c["sgm_depth_refine/three_without_consensus"] = lambda: sgm_depth("_refine", neighbors=3)
    c["sgm_depth_refine/sweep+consensus"] = \
        lambda: sgm_depth("_refine", consensus=1, sw=sweep())
    c["sgm_depth_refine/no_neighbour"] = lambda: sgm_depth("_refine", n_subs=0)
    c["sgm_depth_refine/zero_neighbours"] = lambda: sgm_depth("_refine", neighbors=0)

    # ---- smvs_host_reconstruct_scene_*
    for e in SCENE_ENTRIES:
        c["scene%s/null_dir" % e] = lambda e=e: scene(e, scene_dir=None)
        c["scene%s/null_settings" % e] = lambda e=e: scene(e, settings=False)
    for e in SCENE_FLAG_ENTRIES:
        c["scene%s/bit2" % e] = lambda e=e: scene(e, flags=4)
        c["scene%s/bit5" % e] = lambda e=e: scene(e, flags=32)
        c["scene%s/bit6" % e] = lambda e=e: scene(e, flags=64)
        c["scene%s/all_known+bit6" % e] = lambda e=e: scene(e, flags=1 | 2 | 8 | 16 | 64)
    c["scene_planes/bit5_refine_off"] = lambda: scene("_planes", flags=32, rf=refine(sweeps=0))
    c["scene_planes/bit5+bit6"] = lambda: scene("_planes", flags=32 | 64, rf=refine(sweeps=2))
    c["scene_planes/bit5+null_dir"] = lambda: scene("_planes", flags=32, scene_dir=None)
    c["scene_refine/bit5_refine_on"] = lambda: scene("_refine", flags=32, rf=refine(sweeps=2))
    c["scene_flags/bit2+null_dir"] = lambda: scene("_flags", flags=4, scene_dir=None)
    for e in SCENE_ENTRIES[3:]:
        c["scene%s/steps1" % e] = lambda e=e: scene(e, num_steps=1)
        c["scene%s/steps132+bit2" % e] = lambda e=e: scene(e, num_steps=132, flags=4)
        c["scene%s/steps129+null_dir" % e] = lambda e=e: scene(e, num_steps=129, scene_dir=None)
    for e in SCENE_ENTRIES[5:]:
        c["scene%s/zero_neighbours" % e] = lambda e=e: scene(e, neighbors=0)
        c["scene%s/three_without_consensus" % e] = lambda e=e: scene(e, neighbors=3)
        c["scene%s/seventeen_neighbours" % e] = lambda e=e: scene(e, neighbors=17, consensus=1)
        c["scene%s/neighbours+bit2" % e] = lambda e=e: scene(e, neighbors=0, flags=4)
        c["scene%s/neighbours+steps1" % e] = lambda e=e: scene(e, neighbors=3, num_steps=1)
        c["scene%s/agree_ratio2" % e] = lambda e=e: scene(e, consensus=1, agree_ratio=2.0)
        c["scene%s/agree_ratio_nan" % e] = lambda e=e: scene(e, consensus=1, agree_ratio=NAN)
        c["scene%s/min_agree0" % e] = lambda e=e: scene(e, consensus=1, min_agree=0)
        c["scene%s/min_agree17+steps1" % e] = \
            lambda e=e: scene(e, consensus=1, min_agree=17, num_steps=1)
        c["scene%s/neighbours+agree" % e] = \
            lambda e=e: scene(e, neighbors=17, consensus=1, agree_ratio=-1.0)
    for e in SCENE_ENTRIES[6:]:
        c["scene%s/sweep+consensus" % e] = lambda e=e: scene(e, consensus=1, sw=sweep())
        c["scene%s/sweep+consensus+zero_neighbours" % e] = \
            lambda e=e: scene(e, consensus=1, neighbors=0, sw=sweep())
        c["scene%s/sweep_min_views0" % e] = lambda e=e: scene(e, sw=sweep(min_views=0))
        c["scene%s/sweep_best_k17" % e] = lambda e=e: scene(e, sw=sweep(best_k=17))
        c["scene%s/sweep_cost255" % e] = lambda e=e: scene(e, sw=sweep(support_cost=255))
        c["scene%s/sweep_support-2" % e] = lambda e=e: scene(e, sw=sweep(min_support=-2))
        c["scene%s/sweep_values+steps1" % e] = \
            lambda e=e: scene(e, sw=sweep(min_views=17), num_steps=1)
        c["scene%s/neighbours+sweep_values" % e] = \
            lambda e=e: scene(e, neighbors=17, sw=sweep(best_k=-2))
        c["scene%s/sweep_off_bad_values+bit2" % e] = \
            lambda e=e: scene(e, sw=sweep(on=0, min_views=0), flags=4)
    for e in SCENE_ENTRIES[7:]:
        c["scene%s/uniqueness100" % e] = lambda e=e: scene(e, fl=filt(uniqueness=100))
        c["scene%s/ratio_nan" % e] = lambda e=e: scene(e, fl=filt(speckle_ratio=NAN))
        c["scene%s/filter+steps1" % e] = lambda e=e: scene(e, fl=filt(window=0), num_steps=1)
        c["scene%s/filter+sweep+consensus" % e] = \
            lambda e=e: scene(e, fl=filt(speckle_size=-1), consensus=1, sw=sweep())
        c["scene%s/filter+null_dir" % e] = \
            lambda e=e: scene(e, fl=filt(uniqueness=-1), scene_dir=None)
    for e in SCENE_ENTRIES[8:]:
        c["scene%s/radius4" % e] = lambda e=e: scene(e, ph=photo(radius=4))
        c["scene%s/score2" % e] = lambda e=e: scene(e, ph=photo(radius=1, min_score=2.0))
        c["scene%s/filter+photo" % e] = \
            lambda e=e: scene(e, fl=filt(window=257), ph=photo(witnesses=17))
        c["scene%s/photo+neighbours" % e] = \
            lambda e=e: scene(e, ph=photo(best_k=-1), neighbors=0)
    for e in SCENE_ENTRIES[9:]:
        c["scene%s/sweeps9" % e] = lambda e=e: scene(e, rf=refine(sweeps=9))
        c["scene%s/fill2" % e] = lambda e=e: scene(e, rf=refine(fill=2))
        c["scene%s/photo+refine" % e] = \
            lambda e=e: scene(e, ph=photo(radius=4), rf=refine(samples=9))
        c["scene%s/refine+bit6" % e] = \
            lambda e=e: scene(e, rf=refine(slant_step=NAN), flags=64)
        c["scene%s/refine+steps1" % e] = \
            lambda e=e: scene(e, rf=refine(depth_step=-0.5), num_steps=1)

    # ---- surfaces
    c["surface_script/null_main"] = lambda: surface_script("", main=False)
    c["surface_script/delete_every0"] = lambda: surface_script("", delete_every=0)
    c["surface_script/null_ops"] = lambda: L().smvs_host_surface_script(
        C.byref(A().main), C.byref(A().bundle), fptr(_DEPTH), C.c_int(2), None, C.c_int(1),
        C.c_int(3), iptr(_INFO), dptr(_NODES), bptr(_NV), bptr(_PV))
    c["surface_script/null_info"] = lambda: surface_script("", info=False)
    c["surface_script/unknown_operation"] = \
        lambda: surface_script("", ops=_OPS_UNKNOWN, n_ops=1)
    c["surface_script_planes/null_depth"] = lambda: surface_script("_planes", depth=False)
    c["surface_script_planes/null_slant"] = lambda: surface_script("_planes", slant=False)
    c["surface_script_planes/null_slant+null_main"] = \
        lambda: surface_script("_planes", slant=False, main=False)
    c["surface_script_planes/delete_every0"] = lambda: surface_script("_planes", delete_every=0)
    c["surface_script_planes/unknown_operation"] = \
        lambda: surface_script("_planes", ops=_OPS_UNKNOWN, n_ops=1)
    c["surface_script_device/null_main"] = lambda: surface_script("_device", main=False)
    c["surface_script_device/delete_every0"] = lambda: surface_script("_device", delete_every=0)
    c["surface_script_planes_device/null_depth"] = \
        lambda: surface_script("_planes_device", depth=False)
    c["surface_script_planes_device/null_slant+delete_every0"] = \
        lambda: surface_script("_planes_device", slant=False, delete_every=0)
    c["surface_script_planes_device/null_info"] = \
        lambda: surface_script("_planes_device", info=False)
    c["slant_plane/null"] = lambda: L().smvs_host_slant_plane(
        None, fptr(_SLANT), C.c_int(_W), C.c_int(_H), C.c_int(_W), C.c_int(_H), fptr(_OUT_F))
    c["slant_plane/width0"] = lambda: L().smvs_host_slant_plane(
        fptr(_DEPTH), fptr(_SLANT), C.c_int(_W), C.c_int(_H), C.c_int(0), C.c_int(_H),
        fptr(_OUT_F))
    c["surface_maps/no_subs"] = lambda: surface_maps("", n_subs=0)
    c["surface_maps/null_out"] = lambda: surface_maps("", out=False)
    c["surface_maps_planes/null_depth"] = lambda: surface_maps("_planes", depth=False)
    c["surface_maps_planes/null_slant"] = lambda: surface_maps("_planes", slant=False)
    c["surface_maps_planes/null_slant+no_subs"] = \
        lambda: surface_maps("_planes", slant=False, n_subs=0)
    c["surface_maps_planes/no_subs"] = lambda: surface_maps("_planes", n_subs=0)
    c["surface_maps_host/null_depth"] = lambda: surface_maps("_host", depth=False)
    c["surface_maps_host/null_main"] = lambda: surface_maps("_host", out=False)

    # ---- host-only pieces of the SGM front end
    c["depth_range/null_view"] = lambda: L().smvs_host_depth_range(
        None, C.byref(A().bundle), fptr(_OUT_F))
    c["depth_range/null_bundle"] = lambda: L().smvs_host_depth_range(
        C.byref(A().main), None, fptr(_OUT_F))
    c["reprojection/null_destination"] = lambda: L().smvs_host_reprojection(
        C.byref(A().main), None, fptr(_OUT_F), fptr(_OUT_F[9:]))
    c["reprojection/null_t"] = lambda: L().smvs_host_reprojection(
        C.byref(A().main), C.byref(A().main), fptr(_OUT_F), None)
    c["sgm_image/null_view"] = lambda: L().smvs_host_sgm_image(
        None, C.c_int(1), bptr(_OUT_B), iptr(_OUT_I), iptr(_OUT_I[1:]))
    c["sgm_image/negative_halvings"] = lambda: L().smvs_host_sgm_image(
        C.byref(A().main), C.c_int(-1), bptr(_OUT_B), iptr(_OUT_I), iptr(_OUT_I[1:]))

    # ---- scene and image I/O
    c["scene_info/null_dir"] = lambda: L().smvs_host_scene_info(
        None, b"undistorted", C.c_int(0), iptr(_OUT_I), *([None] * 7))
    c["scene_info/null_embedding"] = lambda: L().smvs_host_scene_info(
        _NOWHERE, None, C.c_int(0), iptr(_OUT_I), *([None] * 7))
    c["scene_info/null_count"] = lambda: L().smvs_host_scene_info(
        _NOWHERE, b"undistorted", C.c_int(0), None, *([None] * 7))
    c["mvei_roundtrip/null_in"] = lambda: L().smvs_host_mvei_roundtrip(None, b"/no/such/out")
    c["mvei_roundtrip/null_out"] = lambda: L().smvs_host_mvei_roundtrip(b"/no/such/in", None)
    c["load_byte_image/null_path"] = lambda: L().smvs_host_load_byte_image(
        None, iptr(_OUT_I), None, C.c_size_t(0))
    c["load_byte_image/null_whc"] = lambda: L().smvs_host_load_byte_image(
        b"/no/such/image.png", None, None, C.c_size_t(0))
    c["save_png/null_path"] = lambda: L().smvs_host_save_png(
        None, bptr(_IMG), C.c_int(_W), C.c_int(_H), C.c_int(1))
    c["save_png/null_pixels"] = lambda: L().smvs_host_save_png(
        b"/no/such/dir/x.png", None, C.c_int(_W), C.c_int(_H), C.c_int(1))
    c["save_png/height0"] = lambda: L().smvs_host_save_png(
        b"/no/such/dir/x.png", bptr(_IMG), C.c_int(_W), C.c_int(0), C.c_int(1))
    c["rescale_half_size_gaussian/null_pixels"] = \
        lambda: L().smvs_host_rescale_half_size_gaussian(
            None, C.c_int(_W), C.c_int(_H), C.c_int(1), bptr(_OUT_B))
    c["rescale_half_size_gaussian/channels0"] = \
        lambda: L().smvs_host_rescale_half_size_gaussian(
            bptr(_IMG), C.c_int(_W), C.c_int(_H), C.c_int(0), bptr(_OUT_B))
    c["rescale_half_size_gaussian_device/null_out"] = \
        lambda: L().smvs_host_rescale_half_size_gaussian_device(
            bptr(_IMG), C.c_int(_W), C.c_int(_H), C.c_int(1), C.c_int(1), C.c_int(0), None,
            C.c_size_t(0), iptr(_OUT_I), iptr(_OUT_I[1:]))
    c["rescale_half_size_gaussian_device/width0"] = \
        lambda: L().smvs_host_rescale_half_size_gaussian_device(
            bptr(_IMG), C.c_int(0), C.c_int(_H), C.c_int(1), C.c_int(1), C.c_int(0),
            bptr(_OUT_B), C.c_size_t(_OUT_B.size), iptr(_OUT_I), iptr(_OUT_I[1:]))

    # ---- the export entries, each with its own name in the text
    for e in EXPORTS:
        c["generate%s/null_dir" % e] = lambda e=e: export(e, scene_dir=None)
        c["generate%s/null_settings" % e] = lambda e=e: export(e, settings=False)
        c["generate%s/null_ids" % e] = lambda e=e: export(e, ids=False, n_ids=1)
    for e in EXPORTS[3:]:
        c["generate%s/null_fused" % e] = lambda e=e: export(e, fused=False)
    c["save_ply_points/null_path"] = lambda: L().smvs_host_save_ply_points(
        None, None, None, None, None, None, C.c_int64(0))
    c["save_ply_points/negative"] = lambda: L().smvs_host_save_ply_points(
        b"/no/such/dir/x.ply", None, None, None, None, None, C.c_int64(-1))
    c["save_ply_points/null_xyz"] = lambda: L().smvs_host_save_ply_points(
        b"/no/such/dir/x.ply", None, fptr(_OUT_F), bptr(_OUT_B), fptr(_OUT_F), fptr(_OUT_F),
        C.c_int64(1))
    c["save_ply_mesh/null_path"] = lambda: L().smvs_host_save_ply_mesh(
        None, None, None, None, None, C.c_int64(0), None, C.c_int64(0))
    c["save_ply_mesh/negative_faces"] = lambda: L().smvs_host_save_ply_mesh(
        b"/no/such/dir/x.ply", None, None, None, None, C.c_int64(0), None, C.c_int64(-1))
    c["save_ply_mesh/null_faces"] = lambda: L().smvs_host_save_ply_mesh(
        b"/no/such/dir/x.ply", fptr(_OUT_F), fptr(_OUT_F), bptr(_OUT_B), fptr(_OUT_F),
        C.c_int64(1), None, C.c_int64(1))

    # ---- COLMAP
    c["undistort_u8/null_pixels"] = lambda: L().smvs_host_undistort_u8(
        None, C.c_int(_W), C.c_int(_H), C.c_int(1), None, f32(1.0), C.c_int(_W), C.c_int(_H),
        C.c_int(-1), bptr(_OUT_B), None)
    c["undistort_u8/null_lens"] = lambda: L().smvs_host_undistort_u8(
        bptr(_IMG), C.c_int(_W), C.c_int(_H), C.c_int(1), None, f32(1.0), C.c_int(_W),
        C.c_int(_H), C.c_int(-1), bptr(_OUT_B), None)
    c["read_colmap_model/null_dir"] = lambda: L().smvs_host_read_colmap_model(
        None, None, C.c_size_t(0), (C.c_uint64 * 3)(), None)
    c["read_colmap_model/null_sizes"] = lambda: L().smvs_host_read_colmap_model(
        b"/no/such/model", None, C.c_size_t(0), None, None)
    c["import_colmap/null_model"] = lambda: L().smvs_host_import_colmap(
        None, b"/no/such/images", _NOWHERE, C.byref(A().imp), None, C.c_int(0),
        C.byref(A().rep), C.c_int(0), None, None, None, None, None)
    c["import_colmap/null_report"] = lambda: L().smvs_host_import_colmap(
        b"/no/such/model", b"/no/such/images", _NOWHERE, C.byref(A().imp), None, C.c_int(0),
        None, C.c_int(0), None, None, None, None, None)
    c["import_colmap/null_ids"] = lambda: L().smvs_host_import_colmap(
        b"/no/such/model", b"/no/such/images", _NOWHERE, C.byref(A().imp), None, C.c_int(1),
        C.byref(A().rep), C.c_int(0), None, None, None, None, None)
    c["import_colmap/negative_room"] = lambda: L().smvs_host_import_colmap(
        b"/no/such/model", b"/no/such/images", _NOWHERE, C.byref(A().imp), None, C.c_int(0),
        C.byref(A().rep), C.c_int(-1), None, None, None, None, None)
    return c


def _run(call):
    """-> (status, text): the slot is thread-local and keeps the last text, so it
    is read right after the failing call."""
    lib = _args().lib
    status = int(call())
    return status, lib.smvs_host_last_error().decode()


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


CASE_IDS = sorted(_golden()) if os.path.exists(GOLDEN) else []


def test_table_and_golden_hold_the_same_cases():
    assert sorted(_build_cases()) == CASE_IDS
    assert len(CASE_IDS) > 300


@pytest.mark.parametrize("case", CASE_IDS)
def test_argument_error(case):
    want = _golden()[case]
    status, text = _run(_build_cases()[case])
    assert status == want["status"] == -1, (case, status, text)
    assert text == want["error"], (case, text)


def test_texts_name_the_entry_that_introduced_the_check():
    """Spot checks of what the JSON records, so that a re-recording cannot quietly
    change the contract: the entry named is the check's, not the caller's."""
    g = _golden()
    assert g["scene_refine/uniqueness100"]["error"].startswith(
        "smvs_host_reconstruct_scene_filtered: ")
    assert g["scene_planes/steps1"]["error"].startswith("smvs_host_reconstruct_scene_steps: ")
    assert g["sgm_depth_refine/photo+refine"]["error"].startswith("smvs_host_sgm_depth_photo: ")
    assert g["sgm_depth_refine/steps130"]["error"].startswith("smvs_host_sgm_depth_steps: ")
    assert g["surface_script_planes/delete_every0"]["error"] \
        == "smvs_host_surface_script: bad argument"
    # the order of the checks
    assert g["scene_refine/filter+steps1"]["error"].startswith(
        "smvs_host_reconstruct_scene_filtered: ")
    assert g["scene_merge/neighbours+bit2"]["error"].startswith(
        "smvs_host_reconstruct_scene_merge: ")
    # the flag masks
    for e in SCENE_FLAG_ENTRIES[:-1]:
        assert g["scene%s/bit5" % e]["error"] == "smvs_host_reconstruct_scene_flags: unknown flag"
    assert g["scene_planes/bit5"]["error"] \
        == "smvs_host_reconstruct_scene_refine: init_slants needs sgm_refine_sweeps > 0"
    for e in SCENE_FLAG_ENTRIES:
        assert g["scene%s/bit6" % e]["error"] == "smvs_host_reconstruct_scene_flags: unknown flag"
    for e in EXPORTS:
        assert g["generate%s/null_dir" % e]["error"] == "smvs_host_generate%s: bad argument" % e


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit("usage: %s --record" % sys.argv[0])
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    out = {}
    for name, call in sorted(_build_cases().items()):
        status, text = _run(call)
        if status != -1:
            sys.exit("%s: status %d, not an argument error" % (name, status))
        out[name] = dict(status=status, error=text)
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded", len(out), "cases in", GOLDEN)
