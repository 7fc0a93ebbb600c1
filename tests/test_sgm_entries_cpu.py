"""The refusals of the 14 view and sweep entries of the SGM front end
(include/smvs_hip.h: smvs_sgm_depth_for_view*, smvs_sgm_sweep_for_view*), one
table: every entry is called directly through ctypes at 24 x 16 with 16 planes,
once per single fault that applies to it, and answers SMVS_ERR_INVALID with a
message that names the argument -- before any device call, so also on a machine
without a GPU.  The expected words are literals: single-fault behaviour is what
csrc/sgm_view.hip's check_sgm_view_call has to keep."""
import ctypes as C

import numpy as np
import pytest

INVALID = -1
W, H, PLANES = 24, 16, 16
NAN = float("nan")

# name: (options the entry takes: None, "mode", "opts", "view" or "sweep"; raw; filtered)
ENTRIES = {
    "smvs_sgm_depth_for_view": (None, False, False),
    "smvs_sgm_depth_for_view_mode": ("mode", False, False),
    "smvs_sgm_depth_for_view_opts": ("opts", False, False),
    "smvs_sgm_depth_for_view_raw": (None, True, False),
    "smvs_sgm_depth_for_view_raw_mode": ("mode", True, False),
    "smvs_sgm_depth_for_view_raw_opts": ("opts", True, False),
    "smvs_sgm_depth_for_view_merge": ("view", False, False),
    "smvs_sgm_depth_for_view_filtered": ("view", False, True),
    "smvs_sgm_depth_for_view_raw_merge": ("view", True, False),
    "smvs_sgm_depth_for_view_raw_filtered": ("view", True, True),
    "smvs_sgm_sweep_for_view": ("sweep", False, False),
    "smvs_sgm_sweep_for_view_filtered": ("sweep", False, True),
    "smvs_sgm_sweep_for_view_raw": ("sweep", True, False),
    "smvs_sgm_sweep_for_view_raw_filtered": ("sweep", True, True),
}
assert len(ENTRIES) == 14


def _lib():
    from smvs_amd import _capi
    lib = _capi.load()
    lib.smvs_last_error.restype = C.c_char_p
    return lib


def _state(entry, consensus):
    """The arguments of a call that passes every check: two neighbours for the
    reference's merge, three otherwise."""
    kind = ENTRIES[entry][0]
    n = 3 if kind == "sweep" or consensus else 2
    return dict(n=n, main_null=False, depth_null=False, w=W, h=H, channels=3, halvings=0,
                sizes=[(W, H)] * 17, nch=[3] * 17, nch_null=False, range=(1.0, 8.0),
                num_steps=PLANES, p1=6, p2=96, opts_null=False, p2_mode=0, winner=0,
                merge=1 if consensus else 0, min_agree=2, agree_ratio=0.95, min_views=1,
                best_k=0, support_cost=20, min_support=0, filter=(0, 1, 0, 0.95),
                checked=False, runner_up=False)


def _call(lib, entry, s):
    from smvs_amd import device
    kind, raw, filtered = ENTRIES[entry]
    u8p, fp, u16p = C.POINTER(C.c_uint8), C.POINTER(C.c_float), C.POINTER(C.c_uint16)
    main = np.full((H, W, 3) if raw else (H, W), 90, np.uint8)
    nb = dict(image=main, M_fwd=np.eye(3), t_fwd=[-6, 0, 0], M_bwd=np.eye(3), t_bwd=[6, 0, 0],
              range_main=[1, 8], range_neighbor=[1, 8])
    keep = []
    arr = device._sgm_neighbors([nb] * 17, keep)    # (room for n_neighbors = 17)
    for k, (nw, nh) in enumerate(s["sizes"]):
        arr[k].width, arr[k].height = nw, nh
    depth = np.zeros((H, W), np.float32)
    checked = np.zeros((17, H, W), np.float32)
    runner = np.zeros((H, W), np.uint16)
    a = [0, None if s["main_null"] else main.ctypes.data_as(u8p), s["w"], s["h"]]
    if raw:
        a += [s["channels"]]
    a += [arr]
    if raw:
        a += [None if s["nch_null"] else (C.c_int * 17)(*s["nch"])]
    a += [s["n"]]
    if raw:
        a += [s["halvings"]]
    if kind == "sweep":
        a += [None if s["range"] is None else (C.c_float * 2)(*s["range"])]
    a += [s["num_steps"], C.c_uint16(s["p1"]), C.c_uint16(s["p2"])]
    opts = {"mode": None, None: None,
            "opts": device.SgmOptions(s["p2_mode"], s["winner"]),
            "view": device.SgmViewOptions(s["p2_mode"], s["winner"], s["merge"], s["min_agree"],
                                          s["agree_ratio"]),
            "sweep": device.SgmSweepOptions(s["p2_mode"], s["winner"], s["min_views"],
                                            s["best_k"], s["support_cost"], s["min_support"])}[kind]
    if kind == "mode":
        a += [s["p2_mode"]]
    elif kind is not None:
        a += [None if s["opts_null"] else C.byref(opts)]
    if filtered:
        filt = None if s["filter"] is None else device.SgmFilterOptions(*s["filter"])
        a += [None if filt is None else C.byref(filt)]
    a += [None if s["depth_null"] else depth.ctypes.data_as(fp)]
    if kind == "view":
        a += [checked.ctypes.data_as(fp) if s["checked"] else None, None]
    elif kind == "sweep" and raw:
        a += [None]
    elif kind == "sweep":
        a += [None, None, None, None]
        if filtered:
            a += [runner.ctypes.data_as(u16p) if s["runner_up"] else None]
    return getattr(lib, entry)(*a)


def _small_neighbor(size):
    return lambda s: s.update(sizes=[(W, H), size] + [(W, H)] * 15)


# (fault, the entries it applies to as a predicate of (kind, raw, filtered),
#  what it changes in the call, a word of the message)
def _faults(kind, consensus):
    reference = kind != "sweep" and not consensus
    many = b"one or two neighbours" if reference else b"n_neighbors"
    return [
        ("null options", lambda k, r, f: k in ("opts", "view", "sweep"),
         lambda s: s.update(opts_null=True), b"null options"),
        ("null filter", lambda k, r, f: f, lambda s: s.update(filter=None), b"null filter"),
        ("unknown p2_mode", lambda k, r, f: k is not None, lambda s: s.update(p2_mode=3),
         b"unknown penalty2 mode"),
        ("unknown winner", lambda k, r, f: k in ("opts", "view", "sweep"),
         lambda s: s.update(winner=2), b"unknown winner"),
        ("unknown merge", lambda k, r, f: k == "view", lambda s: s.update(merge=2),
         b"unknown merge"),
        ("n_neighbors 0", lambda k, r, f: True, lambda s: s.update(n=0), many),
        ("n_neighbors 3, reference", lambda k, r, f: reference, lambda s: s.update(n=3),
         b"one or two neighbours"),
        ("n_neighbors 17", lambda k, r, f: True, lambda s: s.update(n=17), many),
        ("agree_ratio NaN", lambda k, r, f: consensus, lambda s: s.update(agree_ratio=NAN),
         b"agree_ratio"),
        ("min_agree 0", lambda k, r, f: consensus, lambda s: s.update(min_agree=0),
         b"min_agree"),
        ("min_views 0", lambda k, r, f: k == "sweep", lambda s: s.update(min_views=0),
         b"min_views"),
        ("best_k 17", lambda k, r, f: k == "sweep", lambda s: s.update(best_k=17), b"best_k"),
        ("support_cost 255", lambda k, r, f: k == "sweep",
         lambda s: s.update(support_cost=255), b"support_cost"),
        ("min_support n + 1", lambda k, r, f: k == "sweep",
         lambda s: s.update(min_support=s["n"] + 1), b"min_support"),
        ("num_steps 129", lambda k, r, f: True, lambda s: s.update(num_steps=129),
         b"multiple of 8 in [136, 256]"),
        ("penalties (6, 7810), adaptive", lambda k, r, f: k is not None,
         lambda s: s.update(p2_mode=1, p1=6, p2=7810), b"u16"),
        ("null main image", lambda k, r, f: True, lambda s: s.update(main_null=True),
         b"null argument"),
        ("null depth", lambda k, r, f: k != "sweep", lambda s: s.update(depth_null=True),
         b"null argument"),
        ("null neighbor_channels", lambda k, r, f: r, lambda s: s.update(nch_null=True),
         b"null argument"),
        ("channels 2", lambda k, r, f: r, lambda s: s.update(channels=2), b"1 or 3 channels"),
        ("a neighbour's channels 2", lambda k, r, f: r,
         lambda s: s.update(nch=[3, 2] + [3] * 15), b"1 or 3 channels"),
        ("halvings 9", lambda k, r, f: r, lambda s: s.update(halvings=9), b"halvings"),
        ("main image 11 x 8", lambda k, r, f: True, lambda s: s.update(w=11, h=8),
         b"image too small"),
        ("neighbour 10 x 9", lambda k, r, f: k != "sweep", _small_neighbor((10, 9)),
         b"bad neighbour image"),
        ("neighbour 1 x 1", lambda k, r, f: k == "sweep", _small_neighbor((1, 1)),
         b"bad neighbour image"),
        ("range (3, 3)", lambda k, r, f: k == "sweep", lambda s: s.update(range=(3.0, 3.0)),
         b"depth range"),
        ("range NaN", lambda k, r, f: k == "sweep", lambda s: s.update(range=(NAN, 8.0)),
         b"depth range"),
        ("null range", lambda k, r, f: k == "sweep", lambda s: s.update(range=None), b"range"),
        ("checked with the reference merge", lambda k, r, f: k == "view" and reference,
         lambda s: s.update(checked=True), b"consensus merge"),
        ("runner_up with uniqueness 0", lambda k, r, f: k == "sweep" and f and not r,
         lambda s: s.update(runner_up=True), b"runner_up"),
    ]


def _cases():
    for entry, (kind, raw, filtered) in ENTRIES.items():
        for consensus in ((False, True) if kind == "view" else (False,)):
            yield entry, consensus


@pytest.mark.parametrize("entry,consensus", list(_cases()))
def test_every_single_fault_is_refused_without_a_device(entry, consensus):
    lib = _lib()
    kind, raw, filtered = ENTRIES[entry]
    assert hasattr(lib, entry)
    # the call the faults are put into passes every check (it then runs, or
    # finds no device)
    assert _call(lib, entry, _state(entry, consensus)) != INVALID, lib.smvs_last_error()
    count = 0
    for name, applies, change, word in _faults(kind, consensus):
        if not applies(kind, raw, filtered):
            continue
        s = _state(entry, consensus)
        change(s)
        rc = _call(lib, entry, s)
        assert rc == INVALID, (entry, name, rc, lib.smvs_last_error())
        assert word in lib.smvs_last_error(), (entry, name, lib.smvs_last_error())
        count += 1
    assert count >= 8, (entry, count)
    if kind == "sweep":
        # the sweep runs no neighbour-side SGM: a neighbour of 10 x 9 is accepted
        s = _state(entry, consensus)
        _small_neighbor((10, 9))(s)
        assert _call(lib, entry, s) != INVALID, lib.smvs_last_error()


@pytest.mark.parametrize("entry,consensus", list(_cases()))
def test_constant_mode_penalties_are_refused_before_the_device(entry, consensus):
    """penalty2 < penalty1 in the constant mode: SMVS_ERR_INVALID "below
    penalty1" from every entry.  (Before the entries shared one check, the six
    entries that only have the reference's merge -- smvs_sgm_depth_for_view,
    _mode, _opts and their _raw forms -- and the reference merge of the four
    _merge / _filtered entries found this in sgm_run_plan, behind the workspace
    lease and the uploads, so a machine without a GPU answered SMVS_ERR_HIP,
    "no such HIP device"; with a GPU the code and text were these.)"""
    lib = _lib()
    s = _state(entry, consensus)
    s.update(p2_mode=0, p1=40, p2=20)
    assert _call(lib, entry, s) == INVALID, (entry, lib.smvs_last_error())
    assert b"below penalty1" in lib.smvs_last_error(), (entry, lib.smvs_last_error())
