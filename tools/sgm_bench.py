#!/usr/bin/env python3
"""Times smvs_sgm_run on the 960x540x128 workload of BASELINE.json configs[2]
(profiling helper; use under rocprofv3 for per-kernel numbers).
--adaptive-p2: the adaptive-penalty aggregation (SMVS_SGM_P2_ADAPTIVE, the
reference's build without SSE) instead of the constant one; --subplane: the
sub-plane winner (SMVS_SGM_WINNER_SUBPLANE) instead of the plane's depth, and
the distinct depth values of the map; --repeat N: N timed
calls instead of 3; --num-steps N: N inverse-depth planes instead of 128
(2 .. 128, or a multiple of 8 from 136 to 256); --p2 N: penalty2 instead of 96
(above 255: the u16 volume with atomics); --kernels: after one warm-up call,
the per-kernel event times of the timed calls (smvs_sgm_profile) and the path
kernel's share of the HBM peak from its algorithmic bytes.
--neighbors N [--consensus]: instead of one run, a view's whole front end
(smvs_sgm_depth_for_view_opts, or ..._merge with SMVS_SGM_MERGE_CONSENSUS at
agree_ratio 0.95, min_agree 2) over N ring neighbours at the same size: the
time per view and, from smvs_sgm_profile, the left/right-check and merge
kernels (with --consensus the one fused kernel, reported as merge) with the
bytes they move.  Without --consensus N is 1 or 2, the reference's merge.
--neighbors N --sweep: the multi-neighbour plane sweep (smvs_sgm_sweep_for_view
at the defaults for N neighbours) instead: the time per view, the fold kernel
(reported as merge) with its (N + 1) volume bytes against the HBM read peak of
profiles/r2_peaks.json, and the support kernel (reported as lr_check).
--uniqueness U [--uniqueness-window W]: the uniqueness test of include/smvs_hip.h
in the WTA step of every run (U in 1 .. 99; W planes, 1 without the flag);
--speckle N [--speckle-ratio R] (with --neighbors): the speckle removal on the
view's final map (components below N pixels; R 0.95 without the flag), its
launches counted as merge, and the same launches alone on that map
(smvs_sgm_filter_speckles) so that their time stands by itself.
--photo R [--photo-best-k K] [--photo-min-views V] [--photo-min-score S]
[--witnesses N] (with --neighbors): the multi-view photo-consistency test of
include/smvs_hip.h on the view's final map (window radius R in 1 .. 3; K 2, V 2,
S 0.49 without the flags) with N ring views as witnesses, the front end's
neighbours first (N = --neighbors without the flag); its one launch counted as
merge, and the same launch alone on the map in front of it (smvs_sgm_photo_check)
with the bytes it moves, so that its time stands by itself.
--refine SWEEPS [--refine-samples S] (with --photo): the multi-view plane
refinement sweeps of include/smvs_hip.h in the photo test's place (SWEEPS in
1 .. 8; S 2 without the flag; the other options at their defaults), their
1 + 2 SWEEPS + 1 launches counted as merge; in the same session the view with
the photo test alone, and the sweeps alone on the map in front of them
(smvs_sgm_plane_refine) at SWEEPS and at 0 sweeps (the start and the end), so
that the time of one half-sweep launch stands next to the photo kernel's."""
import ctypes as C
import json
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import smvs_amd
from smvs_amd import synth, _capi


def _arg(name, default, kind=int):
    return kind(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


w, h = (1920, 1080) if "--small" not in sys.argv else (480, 270)
main, subs = synth.ring_cameras(w, h, 1)
scene = synth.SphereScene(px_size=3.0 / (1.2 * w))
imgs = [synth.render(scene, c) for c in (main, subs[0])]
half = [im[::2, ::2].copy() for im in imgs]  # stand-in for rescale_half_size
hw, hh = half[0].shape[1], half[0].shape[0]
cm = synth.Camera(main.R, main.t, main.flen, hw, hh)
cs = synth.Camera(subs[0].R, subs[0].t, subs[0].flen, hw, hh)
M, t = synth.reprojection(cm, cs)
adaptive = "--adaptive-p2" in sys.argv
repeat = _arg("--repeat", 3)
D = _arg("--num-steps", 128)
p2 = _arg("--p2", 96)
kernels = "--kernels" in sys.argv
subplane = "--subplane" in sys.argv
kw = dict(adaptive_p2=True) if adaptive else {}
if adaptive:
    print("penalty2 adapted to the intensity step (SMVS_SGM_P2_ADAPTIVE)")
if subplane:
    kw["subplane"] = True
    print("sub-plane winner (SMVS_SGM_WINNER_SUBPLANE)")
uniqueness = _arg("--uniqueness", 0)
speckle = _arg("--speckle", 0)
speckle_ratio = _arg("--speckle-ratio", 0.95, float)
if uniqueness:
    kw.update(uniqueness=uniqueness, uniqueness_window=_arg("--uniqueness-window", 1))
    print("uniqueness test: %d %%, window %d" % (uniqueness, kw["uniqueness_window"]))

photo = _arg("--photo", 0)
refine = _arg("--refine", 0)
if refine and not photo:
    sys.exit("--refine needs --photo (the sweeps use its window and witnesses)")

if "--neighbors" in sys.argv:
    n = _arg("--neighbors", 2)
    consensus = "--consensus" in sys.argv
    sweep = "--sweep" in sys.argv
    if sweep and consensus:
        sys.exit("--sweep and --consensus exclude each other")
    n_all = max(n, _arg("--witnesses", n)) if photo else n
    main, subs = synth.ring_cameras(w, h, n_all)
    small = [im[::2, ::2].copy() for im in [synth.render(scene, c) for c in [main] + subs]]
    cams = [synth.Camera(c.R, c.t, c.flen, hw, hh) for c in [main] + subs]
    nbs = []
    for k in range(1, n_all + 1):
        Mf, tf = synth.reprojection(cams[0], cams[k])
        Mb, tb = synth.reprojection(cams[k], cams[0])
        nbs.append(dict(image=small[k], M_fwd=Mf, t_fwd=tf, M_bwd=Mb, t_bwd=tb,
                        range_main=[2.0, 10.0], range_neighbor=[2.0, 10.0]))
    if consensus:
        kw["consensus"] = True
    if speckle:
        kw.update(speckle_size=speckle, speckle_ratio=speckle_ratio)
        print("speckle removal: components below %d pixels, ratio %g (its launches count as "
              "merge)" % (speckle, speckle_ratio))
    nbs, further = nbs[:n], nbs[n:]
    if photo:
        photo_kw = dict(photo_radius=photo, photo_best_k=_arg("--photo-best-k", 2),
                        photo_min_views=_arg("--photo-min-views", 2),
                        photo_min_score=_arg("--photo-min-score", 0.49, float))
        kw.update(photo_kw, witnesses=further)
        print("photo-consistency test: radius %d, best %d, at least %d views, score >= %g, %d "
              "witnesses (its launch counts as merge)"
              % (photo, photo_kw["photo_best_k"], photo_kw["photo_min_views"],
                 photo_kw["photo_min_score"], n_all))
    if refine:
        refine_kw = dict(refine_sweeps=refine, refine_samples=_arg("--refine-samples", 2))
        kw.update(refine_kw)
        print("plane refinement: %d sweeps, %d samples, defaults otherwise (its launches count "
              "as merge)" % (refine, refine_kw["refine_samples"]))
    print("front end of a view, %d neighbours, %s" % (
        n, "plane sweep (min_views %d, best_k %d, support_cost %d, min_support %d)"
        % smvs_amd.device.sgm_sweep_defaults(n) if sweep
        else "consensus merge (0.95, 2)" if consensus else "the reference's merge"))

    def view():
        if sweep:
            return smvs_amd.sgm_sweep_for_view(small[0], nbs, (2.0, 10.0), D, 6, p2, **kw)["depth"]
        out = smvs_amd.sgm_depth_for_view(small[0], nbs, D, 6, p2, **kw)
        return out["depth"] if isinstance(out, dict) else out

    lib = _capi.load()
    view()   # warm-up: workspace growth, first-launch costs
    times = []
    for i in range(repeat):
        t0 = time.perf_counter()
        out = view()
        times.append(time.perf_counter() - t0)
        print("front end %dx%dx%d x %d neighbours: %.2f ms per view (incl. H2D/D2H), valid %.3f"
              % (hw, hh, D, n, 1e3 * times[-1], (out > 0).mean()))
    print("front end: best %.2f ms per view" % (1e3 * min(times)))
    if refine:
        # the same view with the photo test alone, in this session
        with_sweeps, kw = kw, {k: v for k, v in kw.items() if not k.startswith("refine")}
        view()
        times = []
        for i in range(repeat):
            t0 = time.perf_counter()
            view()
            times.append(time.perf_counter() - t0)
        print("front end with the photo test alone: best %.2f ms per view" % (1e3 * min(times)))
        kw = with_sweeps
    # (the events of the per-kernel timer serialise the launches: a call of its own)
    lib.smvs_sgm_profile(1, None, None)
    for i in range(repeat):
        view()
    ms = (C.c_double * 8)()
    cnt = (C.c_longlong * 8)()
    lib.smvs_sgm_profile(0, ms, cnt)
    names = ["census", "warp", "cost", "paths", "wta", "lr_check", "merge"]
    for i, name in enumerate(names):
        if cnt[i]:
            print("kernel %-8s %9.1f us per launch, %9.1f us per view (%d launches per view)"
                  % (name, 1e3 * ms[i] / cnt[i], 1e3 * ms[i] / repeat, cnt[i] // repeat))
    npix = hw * hh
    if photo:
        # the same launch alone, on the map as it is in front of the test
        plain = {k: v for k, v in kw.items()
                 if not k.startswith(("photo", "speckle", "refine")) and k != "witnesses"}
        if sweep:
            before = smvs_amd.sgm_sweep_for_view(small[0], nbs, (2.0, 10.0), D, 6, p2,
                                                 **plain)["depth"]
        else:
            before = smvs_amd.sgm_depth_for_view(small[0], nbs, D, 6, p2, **plain)
        alone = (photo, photo_kw["photo_best_k"], photo_kw["photo_min_views"],
                 photo_kw["photo_min_score"])
        smvs_amd.sgm_photo_check(small[0], before, nbs + further, *alone)
        lib.smvs_sgm_profile(1, None, None)
        for i in range(repeat):
            after, conf, views = smvs_amd.sgm_photo_check(small[0], before, nbs + further, *alone)
        pms = (C.c_double * 8)()
        pcnt = (C.c_longlong * 8)()
        lib.smvs_sgm_profile(0, pms, pcnt)
        # read: the main image, the map, the witnesses' images (gathered);
        # written: the map, the confidence, the views
        nbytes = npix * (1 + 4 + n_all + 4 + 4 + 1)
        samples = int((before > 0).sum()) * n_all * (2 * photo + 1) ** 2
        us = 1e3 * pms[6] / repeat
        print("photo test alone (%d launch): %.1f us per map, %.1f MB, %.3f TB/s; at most %.1f M "
              "samples; %d of %d valid pixels removed, views up to %d"
              % (pcnt[6] // repeat, us, nbytes / 1e6, nbytes / us / 1e6, samples / 1e6,
                 int(((before > 0) & (after == 0)).sum()), int((before > 0).sum()),
                 int(views.max())))
    if refine:
        # the sweeps alone on the same map: all launches, and the start and the
        # end alone (0 sweeps); the difference is the 2 x sweeps half-sweeps
        def alone_us(sweeps):
            args = dict(sweeps=sweeps, samples=refine_kw["refine_samples"])
            smvs_amd.sgm_plane_refine(small[0], before, nbs + further, *alone, **args)
            lib.smvs_sgm_profile(1, None, None)
            for i in range(repeat):
                got = smvs_amd.sgm_plane_refine(small[0], before, nbs + further, *alone, **args)
            rms = (C.c_double * 8)()
            rcnt = (C.c_longlong * 8)()
            lib.smvs_sgm_profile(0, rms, rcnt)
            return 1e3 * rms[6] / repeat, rcnt[6] // repeat, got
        ends_us, ends_n, _ = alone_us(0)
        all_us, all_n, (rout, rslant, rconf, rviews) = alone_us(refine)
        valid = before > 0
        print("refinement alone (%d launches): %.1f us per map; start + end (%d launches): %.1f "
              "us; a half-sweep launch: %.1f us (the photo kernel: %.1f us); %d of %d valid "
              "pixels changed depth, %d of %d holes filled, %d pixels without a depth after "
              "(photo test alone: %d)"
              % (all_n, all_us, ends_n, ends_us, (all_us - ends_us) / (2 * refine), us,
                 int((valid & (rout != before) & (rout != 0)).sum()), int(valid.sum()),
                 int((~valid & (rout > 0)).sum()), int((~valid).sum()),
                 int((rout == 0).sum()), int((after == 0).sum())))
    if speckle and not photo:
        # the same launches alone, on the map as it is in front of the filter
        plain = {k: v for k, v in kw.items() if not k.startswith("speckle")}
        if sweep:
            before = smvs_amd.sgm_sweep_for_view(small[0], nbs, (2.0, 10.0), D, 6, p2,
                                                 **plain)["depth"]
        else:
            before = smvs_amd.sgm_depth_for_view(small[0], nbs, D, 6, p2, **plain)
        smvs_amd.sgm_filter_speckles(before, speckle, speckle_ratio)
        lib.smvs_sgm_profile(1, None, None)
        for i in range(repeat):
            after, size = smvs_amd.sgm_filter_speckles(before, speckle, speckle_ratio)
        sms = (C.c_double * 8)()
        scnt = (C.c_longlong * 8)()
        lib.smvs_sgm_profile(0, sms, scnt)
        print("speckle removal alone (%d launches): %.1f us per map; %d of %d valid pixels "
              "removed, largest component %d" % (scnt[6] // repeat, 1e3 * sms[6] / repeat,
                                                 int(((before > 0) & (after == 0)).sum()),
                                                 int((before > 0).sum()), int(size.max())))
    if photo:
        print("merge class: %d launches per view, the %s%s among them: %.1f us per view"
              % (cnt[6] // repeat, "refinement's" if refine else "photo test",
                 " and the speckle launches" if speckle else "",
                 1e3 * ms[6] / repeat))
    elif speckle:
        print("merge class: %d launches per view, the speckle launches among them: %.1f us per "
              "view" % (cnt[6] // repeat, 1e3 * ms[6] / repeat))
    elif sweep:
        # n volumes read, the folded one written
        nbytes = (n + 1) * npix * D
        us = 1e3 * ms[6] / max(cnt[6], 1)
        with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                               "profiles", "r2_peaks.json")) as f:
            peak = json.load(f)["hbm_read_GBps"] / 1e3
        print("fold (one kernel): %.1f us per view, %.1f MB, %.2f TB/s, %.2f of the %.2f TB/s "
              "HBM read peak" % (us, nbytes / 1e6, nbytes / us / 1e6, nbytes / us / 1e6 / peak,
                                 peak))
    if sweep:
        print("support (one kernel): %.1f us per view" % (1e3 * ms[5] / max(cnt[5], 1)))
    elif speckle or photo:
        pass
    elif consensus:
        # n forward maps read, n scattered lookups, the merged map written
        nbytes = 4 * npix * (2 * n + 1)
        us = 1e3 * ms[6] / max(cnt[6], 1)
        print("check + merge (one kernel): %.1f us per view, %.1f MB, %.2f TB/s"
              % (1e3 * ms[6] / repeat, nbytes / 1e6, nbytes / us / 1e6))
    else:
        # per check a map read and written back where rejected, a lookup; the
        # merge reads two maps and writes one
        print("check + merge (%d launches): %.1f us per view"
              % ((cnt[5] + cnt[6]) // repeat, 1e3 * (ms[5] + ms[6]) / repeat))
    sys.exit(0)


def run():
    return smvs_amd.sgm_run(half[0], half[1], M.astype(np.float32), t.astype(np.float32),
                            2.0, 10.0, D, 6, p2, **kw)


lib = _capi.load()
if kernels:
    run()   # warm-up: workspace growth, first-launch costs
    lib.smvs_sgm_profile(1, None, None)
for i in range(repeat):
    t0 = time.perf_counter()
    out = run()
    dt = time.perf_counter() - t0
    print("sgm_run %dx%dx%d: %.1f ms (incl. H2D/D2H), valid %.2f" % (hw, hh, D, 1e3 * dt, (out["depth"] > 0).mean()))
if subplane:
    print("distinct depth values: %d" % np.unique(out["depth"][out["depth"] > 0]).size)
if kernels:
    ms = (C.c_double * 8)()
    cnt = (C.c_longlong * 8)()
    lib.smvs_sgm_profile(0, ms, cnt)
    names = ["census", "warp", "cost", "paths", "wta"]
    for i, name in enumerate(names):
        if cnt[i]:
            print("kernel %-6s %9.1f us per call (%d launches)" % (name, 1e3 * ms[i] / cnt[i], cnt[i]))
    if cnt[3]:
        # each of the eight directions reads C once and writes one byte per cell
        # (penalty2 <= 255), or adds a u16 to S (read + write) otherwise
        cells = hw * hh * D
        nbytes = 8 * cells * (2 if p2 <= 255 else 5)
        us = 1e3 * ms[3] / cnt[3]
        print("paths: %.1f MB algorithmic, %.2f TB/s, %.2f of the 8 TB/s HBM peak"
              % (nbytes / 1e6, nbytes / us / 1e6, nbytes / us / 1e6 / 8.0))
