"""ctypes handle on the C++ host mirror (csrc/host/libsmvs_host.so):
smvs_amd::DepthOptimizer::optimize and the SGM initialisation, driven with
the inputs of smvs_amd.synth.pipeline_inputs()."""
import ctypes as C
import os

import numpy as np

from . import _capi

HOST_LIB = os.path.join(_capi.HERE, "csrc", "host", "libsmvs_host.so")
_lib = None

_fp = C.POINTER(C.c_float)
_u8p = C.POINTER(C.c_uint8)
_i32p = C.POINTER(C.c_int32)


class HostView(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("channels", C.c_int),
                ("bytes", _u8p), ("flen", C.c_float), ("rot", C.c_float * 9),
                ("trans", C.c_float * 3), ("view_id", C.c_int)]


class HostBundle(C.Structure):
    _fields_ = [("num_features", C.c_int), ("positions", _fp),
                ("ref_offsets", _i32p), ("ref_views", _i32p)]


class HostOptions(C.Structure):
    _fields_ = [("regularization", C.c_double),
                ("light_surf_regularization", C.c_double),
                ("num_iterations", C.c_int), ("min_scale", C.c_int),
                ("use_shading", C.c_int), ("use_sgm", C.c_int),
                ("full_optimization", C.c_int), ("device", C.c_int),
                ("solver", C.c_int), ("gamma_correction", C.c_int)]


class HostLog(C.Structure):
    _fields_ = [("count", C.c_int), ("scale", C.c_int * 256),
                ("iter", C.c_int * 256), ("newton_steps", C.c_int * 256),
                ("valid_patches", C.c_int * 256), ("cg_iterations", C.c_int * 256),
                ("active_patch_steps", C.c_longlong * 256),
                ("loop_seconds", C.c_double * 256),
                ("has_lighting", C.c_int), ("lighting", C.c_double * 16)]


def load():
    global _lib
    if _lib is None:
        _capi.load()  # libsmvs_hip.so first
        if not os.path.exists(HOST_LIB):
            raise _capi.SmvsError(-2, "host library %s is missing" % HOST_LIB)
        _lib = C.CDLL(HOST_LIB)
        _lib.smvs_host_last_error.restype = C.c_char_p
    return _lib


def _view(img, cam, view_id, keep):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    if img.ndim == 2:
        img = img[:, :, None]
    keep.append(img)
    v = HostView()
    v.height, v.width, v.channels = img.shape
    v.bytes = img.ctypes.data_as(_u8p)
    v.flen = cam.flen
    for i, x in enumerate(np.asarray(cam.R, dtype=np.float32).reshape(9)):
        v.rot[i] = float(x)
    for i, x in enumerate(np.asarray(cam.t, dtype=np.float32).reshape(3)):
        v.trans[i] = float(x)
    v.view_id = view_id
    return v


def _marshal(inputs, keep):
    cams, images = inputs["cams"], inputs["images"]
    main = _view(images[0], cams[0], inputs["view_ids"][0], keep)
    n_subs = len(cams) - 1
    subs = (HostView * n_subs)()
    for j in range(n_subs):
        subs[j] = _view(images[j + 1], cams[j + 1], inputs["view_ids"][j + 1], keep)
    feats = np.ascontiguousarray(inputs["features"], dtype=np.float32).reshape(-1, 3)
    nf = feats.shape[0]
    offsets = (np.arange(nf + 1) * len(cams)).astype(np.int32)
    refs = np.tile(np.asarray(inputs["view_ids"], dtype=np.int32), nf)
    keep += [feats, offsets, refs]
    b = HostBundle(nf, feats.ctypes.data_as(_fp), offsets.ctypes.data_as(_i32p),
                   refs.ctypes.data_as(_i32p))
    return main, subs, n_subs, b


def optimize(inputs, regularization=0.01, light_reg=0.0, num_iterations=5,
             min_scale=2, use_shading=False, sgm_depth=None,
             full_optimization=False, device=0, solver="auto", want_maps=True,
             gamma_correction=False, device_shading_prep=False, sgm_slant=None,
             init_slants=False):
    """want_maps=False: optimize() only -- the depth / normal maps the reference
    reads back with get_depth() / get_normals() afterwards are not fetched (the
    embeddings optimize() itself writes are; tools/optimize_timeline.py).
    device_shading_prep (with use_shading): the main view's shading planes are
    made on the device (smvs_ctx_prepare_shading) instead of by the host's
    StereoView::initialize_linear, with the same bits; off by default.
    sgm_slant (dm_h x dm_w x 2, z-depth per SGM pixel, as the SGM front end's
    refinement sweeps give it) is stored as the view's smvs-sgm-slant embedding;
    init_slants (DepthOptimizer::Options::init_slants): the initial surface's node
    slopes come from it.  init_slants without sgm_depth, or without slants of two
    channels and sgm_depth's size, is an error; off by default."""
    lib = load()
    keep = []
    main, subs, n_subs, b = _marshal(inputs, keep)
    o = HostOptions(regularization, light_reg, num_iterations, min_scale,
                    1 if use_shading else 0, 1 if sgm_depth is not None else 0,
                    1 if full_optimization else 0, device,
                    dict(auto=0, streaming=1, resident_ref=2)[solver],
                    1 if gamma_correction else 0)
    h, w = main.height, main.width
    depth = np.zeros((h, w), dtype=np.float32)
    normals = np.zeros((h, w, 3), dtype=np.float32)
    log = HostLog()
    sd = rt = None
    sw = sh = 0
    if sgm_depth is not None:
        sd = np.ascontiguousarray(sgm_depth, dtype=np.float32)
        sh, sw = sd.shape
        rt = np.zeros_like(sd)
    if sgm_slant is None and not init_slants:
        rc = lib.smvs_host_optimize_flags(C.byref(main), subs, n_subs, C.byref(b),
            sd.ctypes.data_as(_fp) if sd is not None else None, sw, sh,
            rt.ctypes.data_as(_fp) if rt is not None else None, C.byref(o),
            C.c_uint(1 if device_shading_prep else 0),
            depth.ctypes.data_as(_fp) if want_maps else None,
            normals.ctypes.data_as(_fp) if want_maps else None, C.byref(log))
    else:
        sl = None
        slw = slh = slc = 0
        if sgm_slant is not None:
            sl = np.ascontiguousarray(sgm_slant, dtype=np.float32)
            if sl.ndim == 2:
                sl = sl[:, :, None]
            slh, slw, slc = sl.shape
        rc = lib.smvs_host_optimize_planes(C.byref(main), subs, n_subs, C.byref(b),
            sd.ctypes.data_as(_fp) if sd is not None else None, sw, sh,
            rt.ctypes.data_as(_fp) if rt is not None else None,
            sl.ctypes.data_as(_fp) if sl is not None else None, C.c_int(slw), C.c_int(slh),
            C.c_int(slc), C.byref(o),
            C.c_uint((1 if device_shading_prep else 0) | (2 if init_slants else 0)),
            depth.ctypes.data_as(_fp) if want_maps else None,
            normals.ctypes.data_as(_fp) if want_maps else None, C.byref(log))
    if rc != 0:
        raise _capi.SmvsError(rc, lib.smvs_host_last_error().decode())
    steps = [dict(scale=log.scale[i], iter=log.iter[i],
                  newton_steps=log.newton_steps[i],
                  valid_patches=log.valid_patches[i],
                  cg_iterations=log.cg_iterations[i],
                  active_patch_steps=log.active_patch_steps[i],
                  loop_seconds=log.loop_seconds[i]) for i in range(log.count)]
    return dict(depth=depth if want_maps else None,
                normals=normals if want_maps else None, log=steps, sgm_roundtrip=rt,
                lighting=np.array(log.lighting[:]) if log.has_lighting else None)


def optimize_views(inputs, n_jobs, regularization=0.01, light_reg=0.0,
                   num_iterations=5, min_scale=2, use_shading=False, sgm_scale=None,
                   first_device=0, num_devices=1, views_in_flight=1, solver="auto",
                   keep_job=0):
    """n_jobs reference views (each job the same scene: main + neighbours of
    `inputs`) through smvs_amd::ViewQueue -- the per-view tasks of smvsrecon
    (app/smvsrecon.cc:658-733): StereoViews, SGM front end (sgm_scale is not
    None), DepthOptimizer::optimize, depth + normal maps.  Returns the maps of
    job `keep_job`, the per-job logs and wall times."""
    lib = load()
    keep = []
    main, subs, n_subs, b = _marshal(inputs, keep)
    mains = (HostView * n_jobs)(*([main] * n_jobs))
    all_subs = (HostView * (n_jobs * n_subs))()
    for j in range(n_jobs):
        for k in range(n_subs):
            all_subs[j * n_subs + k] = subs[k]
    o = HostOptions(regularization, light_reg, num_iterations, min_scale,
                    1 if use_shading else 0, 1 if sgm_scale is not None else 0,
                    0, first_device, dict(auto=0, streaming=1, resident_ref=2)[solver], 0)
    h, w = main.height, main.width
    depth = np.zeros((h, w), dtype=np.float32)
    normals = np.zeros((h, w, 3), dtype=np.float32)
    secs = np.zeros(n_jobs)
    total = C.c_double(0.0)
    logs = (HostLog * n_jobs)()
    rc = lib.smvs_host_optimize_views(mains, all_subs, C.c_int(n_jobs), C.c_int(n_subs),
        C.byref(b), C.byref(o), C.c_int(-1 if sgm_scale is None else sgm_scale),
        C.c_int(first_device), C.c_int(num_devices), C.c_int(views_in_flight),
        C.c_int(keep_job), depth.ctypes.data_as(_fp), normals.ctypes.data_as(_fp),
        secs.ctypes.data_as(C.POINTER(C.c_double)), C.byref(total), logs)
    if rc != 0:
        raise _capi.SmvsError(rc, lib.smvs_host_last_error().decode())
    out_logs = [[dict(scale=l.scale[i], iter=l.iter[i], newton_steps=l.newton_steps[i],
                      valid_patches=l.valid_patches[i], cg_iterations=l.cg_iterations[i],
                      active_patch_steps=l.active_patch_steps[i],
                      loop_seconds=l.loop_seconds[i])
                 for i in range(l.count)] for l in logs]
    return dict(depth=depth, normals=normals, logs=out_logs, job_seconds=secs,
                total_seconds=total.value, views_per_s=n_jobs / total.value)


def gn_solve_step(inputs, init_scale, regularization=0.01, device=0):
    """One construct + solve through the compatibility classes
    smvs_amd::GaussNewtonStep / ConjugateGradient (reference signatures,
    lib/gauss_newton_step.h:40-50, lib/conjugate_gradient.h:55-56) on the
    surface Surface::create builds at init_scale.  Returns the planes and
    reprojections the step used (to feed the oracle the same inputs), the
    surface, g, x, H9, P and the solver's status."""
    lib = load()
    keep = []
    main, subs, n_subs, b = _marshal(inputs, keep)
    surf = surface_script(inputs, init_scale, [])
    h, w = main.height, main.width
    N = (surf["npx"] + 1) * (surf["npy"] + 1)
    mg = np.zeros((h, w, 2), np.float32)
    sg = np.zeros((n_subs, h, w, 2), np.float32)
    sh = np.zeros((n_subs, h, w, 3), np.float32)
    M = np.zeros((n_subs, 9)); t = np.zeros((n_subs, 3)); fl = np.zeros(2, np.float32)
    g = np.zeros(4 * N); x = np.zeros(4 * N); H9 = np.zeros((N, 9, 16)); P = np.zeros((N, 16))
    cg = np.zeros(2, np.int32)
    dp = C.POINTER(C.c_double)
    rc = lib.smvs_host_gn_solve_step(C.byref(main), subs, C.c_int(n_subs), C.byref(b),
        C.c_int(init_scale), C.c_double(regularization), C.c_int(device),
        mg.ctypes.data_as(_fp), sg.ctypes.data_as(_fp), sh.ctypes.data_as(_fp),
        M.ctypes.data_as(dp), t.ctypes.data_as(dp), fl.ctypes.data_as(_fp),
        g.ctypes.data_as(dp), x.ctypes.data_as(dp), H9.ctypes.data_as(dp),
        P.ctypes.data_as(dp), cg.ctypes.data_as(_i32p))
    if rc != 0:
        raise _capi.SmvsError(rc, lib.smvs_host_last_error().decode())
    surf.update(width=w, height=h,
                patch_vis=np.where(surf["patch_valid"] != 0, (1 << n_subs) - 1, 0).astype(np.uint32))
    views = dict(flen=float(fl[0]), inv_flen=float(fl[1]), grad=mg,
                 subs=[(sg[j], sh[j]) for j in range(n_subs)], M=M, t=t,
                 shading=None, shading_grad=None)
    return dict(surf=surf, views=views, g=g, x=x, H9=H9, P=P,
                iterations=int(cg[0]), info=int(cg[1]))


class ReconSettings(C.Structure):
    _fields_ = [("image_embedding", C.c_char_p), ("regularization", C.c_float),
                ("output_scale", C.c_int), ("use_shading", C.c_int), ("use_sgm", C.c_int),
                ("force_recon", C.c_int), ("force_sgm", C.c_int),
                ("full_optimization", C.c_int), ("sgm_min", C.c_float),
                ("sgm_max", C.c_float), ("sgm_scale", C.c_int), ("num_neighbors", C.c_int),
                ("min_neighbors", C.c_int), ("first_device", C.c_int),
                ("num_devices", C.c_int), ("views_in_flight", C.c_int),
                ("input_scale", C.c_int), ("max_pixels", C.c_int)]


class SgmSweep(C.Structure):
    """smvs_host_sgm_sweep of csrc/host/host_capi.h."""
    _fields_ = [("sweep", C.c_int), ("min_views", C.c_int), ("best_k", C.c_int),
                ("support_cost", C.c_int), ("min_support", C.c_int)]


class SgmFilter(C.Structure):
    """smvs_host_sgm_filter of csrc/host/host_capi.h: ReconSettings::
    sgm.uniqueness / uniqueness_window / speckle_size / speckle_ratio
    (SGMStereo::Options::uniqueness / ...), passed next to the settings struct,
    which keeps its layout."""
    _fields_ = [("uniqueness", C.c_int), ("uniqueness_window", C.c_int),
                ("speckle_size", C.c_int), ("speckle_ratio", C.c_float)]


class SgmPhoto(C.Structure):
    """smvs_host_sgm_photo of csrc/host/host_capi.h: ReconSettings::
    sgm.photo_radius / photo_best_k / photo_min_views / photo_min_score /
    photo_witnesses (SGMStereo::Options::photo_radius / ...), passed next to
    the settings struct, which keeps its layout."""
    _fields_ = [("radius", C.c_int), ("best_k", C.c_int), ("min_views", C.c_int),
                ("min_score", C.c_float), ("witnesses", C.c_int)]


class SgmRefine(C.Structure):
    """smvs_host_sgm_refine of csrc/host/host_capi.h: ReconSettings::
    sgm.refine_sweeps / refine_samples / refine_depth_step /
    refine_slant_step / refine_seed / refine_fill (SGMStereo::Options::
    refine_sweeps / ...), passed next to the settings struct, which keeps its
    layout."""
    _fields_ = [("sweeps", C.c_int), ("samples", C.c_int), ("depth_step", C.c_float),
                ("slant_step", C.c_float), ("seed", C.c_uint32), ("fill", C.c_int)]


def reconstruct_scene(scene_dir, view_ids=None, image_embedding="undistorted",
                      regularization=1.0, output_scale=2, use_shading=False, use_sgm=True,
                      force_recon=False, force_sgm=False, sgm_range=(0.0, 0.0), sgm_scale=1,
                      num_neighbors=6, min_neighbors=3, first_device=0, num_devices=1,
                      views_in_flight=2, input_scale=-1, max_pixels=1700000, details=False,
                      sgm_adaptive_penalty2=False, device_input_scaling=False,
                      device_shading_prep=False, gamma_correction=False, sgm_num_steps=128,
                      sgm_subplane=False, sgm_neighbors=2, sgm_consensus=False,
                      sgm_agree_ratio=0.95, sgm_min_agree=2, sgm_sweep=False,
                      sgm_sweep_min_views=-1, sgm_sweep_best_k=-1, sgm_sweep_support_cost=20,
                      sgm_sweep_min_support=-1, sgm_uniqueness=0, sgm_uniqueness_window=1,
                      sgm_speckle_size=0, sgm_speckle_ratio=0.95, sgm_photo_radius=0,
                      sgm_photo_best_k=2, sgm_photo_min_views=2, sgm_photo_min_score=0.49,
                      sgm_photo_witnesses=-1, sgm_refine_sweeps=0, sgm_refine_samples=2,
                      sgm_refine_depth_step=0.02, sgm_refine_slant_step=0.01,
                      sgm_refine_seed=1, sgm_refine_fill=1, init_slants=False):
    """smvsrecon's scene-level run (app/smvsrecon.cc:400-745) through
    smvs_amd::reconstruct_scene: returns (reconstructed ids, skipped, seconds)
    [, input scale used if `details`].  input_scale < 0 (the default, as
    app/smvsrecon.cc:44): smvsrecon's automatic choice from max_pixels
    (:477-500); 0: full resolution; > 0: the views are read from the
    embedding undist-L<input_scale>, created with rescale_half_size_gaussian
    where missing (:621-650), and the outputs are named smvs-B<input_scale>.
    sgm_adaptive_penalty2: the SGM front end as the reference's build without
    SSE runs it (lib/sgm_stereo.cc:310-346); off by default.
    device_input_scaling: the undist-L<input_scale> images are made on the
    device (smvs_rescale_half_gaussian, one ViewQueue task per view) instead of
    by the host loop, with the same bytes; off by default.
    device_shading_prep (with use_shading): every view's shading planes are made
    on the device (smvs_ctx_prepare_shading) instead of by the host's
    StereoView::initialize_linear, with the same bits; off by default.
    gamma_correction: smvsrecon's --gamma-srgb (app/smvsrecon.cc:52, 669), with
    use_shading only.
    sgm_num_steps: the inverse-depth planes of the SGM front end
    (SGMStereo::Options::num_steps): 2 .. 128, or a multiple of 8 from 136 to
    256; smvsrecon runs 128.
    sgm_subplane: ReconSettings::sgm.subplane -- the smvs-sgm map of every view
    refined between the planes (SGMStereo::Options::subplane); off by default.
    An smvs-sgm embedding of the right size is reused as before
    (app/smvsrecon.cc:702-708): switching the mode on for a scene that has been
    reconstructed already needs force_sgm as well.
    sgm_neighbors, sgm_consensus, sgm_agree_ratio, sgm_min_agree:
    ReconSettings::sgm.num_neighbors / ... -- the smvs-sgm map of every view from its
    first sgm_neighbors neighbours (capped by the neighbours the view has, which
    num_neighbors bounds), merged by consensus (SGMStereo::Options::consensus,
    SMVS_SGM_MERGE_CONSENSUS of include/smvs_hip.h); more than two neighbours
    without sgm_consensus is an error.  Off by default; 0.95 and 2 are defaults of
    a user option, not tuned values, and nobody has measured their effect on real
    scenes.  The reuse rule is that of sgm_subplane (force_sgm).
    sgm_sweep and its four values: ReconSettings::sgm.sweep / ... -- the smvs-sgm
    map of every view by the multi-neighbour plane sweep of include/smvs_hip.h
    over its first sgm_neighbors neighbours (one cost volume from all of them,
    one aggregation, one winner, a support test; no left/right check) instead of
    the runs and the merge; not together with sgm_consensus.  -1: the default at
    n neighbours (min_views min(2, n), best_k (n + 1) // 2, min_support
    min(2, n)).  Off by default; these and 20 are defaults of a user option,
    untuned, and nobody has measured them on real scenes.  The reuse rule is that
    of sgm_subplane (force_sgm).
    sgm_uniqueness, sgm_uniqueness_window, sgm_speckle_size, sgm_speckle_ratio:
    ReconSettings::sgm.uniqueness / ... -- the two filters of include/smvs_hip.h
    in every view's SGM front end, whichever of the three it is: the uniqueness
    test (0 .. 99, a percentage; 0 is off) over planes more than the window
    (1 .. 256) from the winner in every run, and the removal of connected
    components of fewer than sgm_speckle_size pixels (0 and 1 are off) from the
    final map.  Off by default; (0, 1, 0, 0.95) are defaults of a user option,
    untuned, and nobody has measured them on real scenes.  The reuse rule is that
    of sgm_subplane (force_sgm).
    sgm_photo_radius, sgm_photo_best_k, sgm_photo_min_views, sgm_photo_min_score,
    sgm_photo_witnesses: ReconSettings::sgm.photo_radius / ... -- the multi-view
    photo-consistency test of include/smvs_hip.h behind every view's SGM front
    end, whichever of the three it is, before the speckle removal: radius 1 .. 3
    (0 is off), the view's first sgm_photo_witnesses neighbours as witnesses (-1:
    all num_neighbors of them), the mean of the best_k largest scores, none with
    fewer than min_views, no depth below min_score.  The confidence is saved as
    smvs-sgm-confidence next to smvs-sgm.  Off by default; (0, 2, 2, 0.49, -1) are
    defaults of a user option, untuned, and nobody has measured them on real
    scenes.  The reuse rule is that of sgm_subplane (force_sgm).
    sgm_refine_sweeps, sgm_refine_samples, sgm_refine_depth_step,
    sgm_refine_slant_step, sgm_refine_seed, sgm_refine_fill: ReconSettings::
    sgm.refine_sweeps / ... -- the multi-view plane refinement sweeps of
    include/smvs_hip.h in the photo test's place (they need sgm_photo_radius > 0):
    1 .. 8 red-black sweeps (0 is off) in which a pixel adopts a neighbour's plane
    or one of `samples` perturbations of its own whenever that raises its
    confidence.  The slants are saved as smvs-sgm-slant (two channels) next to
    smvs-sgm-confidence; the optimizer reads them with init_slants only.  Off by
    default; (0, 2, 0.02, 0.01, 1, 1) are defaults of a user option, untuned, and
    nobody has measured them on real scenes.  The reuse rule is that of
    sgm_subplane (force_sgm).
    init_slants: ReconSettings::init_slants -- every view's initial surface takes
    its node slopes from the view's smvs-sgm-slant embedding (include/smvs_hip.h,
    "Node slopes from the SGM plane hypotheses").  With sgm_refine_sweeps=0 it is
    an error; off by default, and its effect on real scenes is not measured."""
    if init_slants and int(sgm_refine_sweeps) == 0:
        raise ValueError("init_slants needs sgm_refine_sweeps > 0")
    lib = load()
    filt = SgmFilter(int(sgm_uniqueness), int(sgm_uniqueness_window), int(sgm_speckle_size),
                     float(sgm_speckle_ratio))
    photo = SgmPhoto(int(sgm_photo_radius), int(sgm_photo_best_k), int(sgm_photo_min_views),
                     float(sgm_photo_min_score), int(sgm_photo_witnesses))
    refine = SgmRefine(int(sgm_refine_sweeps), int(sgm_refine_samples),
                       float(sgm_refine_depth_step), float(sgm_refine_slant_step),
                       int(sgm_refine_seed) & 0xFFFFFFFF, int(sgm_refine_fill))
    sweep = SgmSweep(1 if sgm_sweep else 0, sgm_sweep_min_views, sgm_sweep_best_k,
                     sgm_sweep_support_cost, sgm_sweep_min_support)
    st = ReconSettings(image_embedding.encode(), regularization, output_scale,
                       1 if use_shading else 0, 1 if use_sgm else 0,
                       1 if force_recon else 0, 1 if force_sgm else 0, 0,
                       sgm_range[0], sgm_range[1], sgm_scale, num_neighbors, min_neighbors,
                       first_device, num_devices, views_in_flight, input_scale, max_pixels)
    ids = None if view_ids is None else np.asarray(view_ids, dtype=np.int32)
    # (room for every view of the scene: smvs_host_scene_info)
    cap = C.c_int(0)
    lib.smvs_host_scene_info(scene_dir.encode(), image_embedding.encode(), C.c_int(0),
                             C.byref(cap), None, None, None, None, None, None, None)
    out = np.zeros(max(cap.value, 1), np.int32)
    n = C.c_int(0); sk = C.c_int(0); secs = C.c_double(0.0); used = C.c_int(0)
    entry = lib.smvs_host_reconstruct_scene_planes if init_slants \
        else lib.smvs_host_reconstruct_scene_refine
    rc = entry(scene_dir.encode(), C.byref(st),
        C.c_uint((1 if sgm_adaptive_penalty2 else 0) | (2 if device_input_scaling else 0)
                 | (8 if device_shading_prep else 0) | (16 if gamma_correction else 0)
                 | (32 if init_slants else 0)),
        C.c_int(sgm_num_steps), C.c_int(1 if sgm_subplane else 0),
        C.c_int(sgm_neighbors), C.c_int(1 if sgm_consensus else 0),
        C.c_float(sgm_agree_ratio), C.c_int(sgm_min_agree), C.byref(sweep), C.byref(filt),
        C.byref(photo), C.byref(refine),
        ids.ctypes.data_as(_i32p) if ids is not None else None,
        C.c_int(0 if ids is None else ids.size), out.ctypes.data_as(_i32p),
        C.c_int(out.size), C.byref(n), C.byref(sk), C.byref(secs), C.byref(used))
    if rc != 0:
        raise _capi.SmvsError(rc, lib.smvs_host_last_error().decode())
    res = ([int(x) for x in out[:min(n.value, out.size)]], sk.value, secs.value)
    return res + (used.value,) if details else res


def load_byte_image(path):
    """A u8 image embedding (.png via csrc/host/png_io.cc, or .mvei)."""
    lib = load()
    whc = (C.c_int * 3)()
    rc = lib.smvs_host_load_byte_image(path.encode(), whc, None, C.c_size_t(0))
    if rc != 0:
        raise _capi.SmvsError(rc, lib.smvs_host_last_error().decode())
    w, h, c = whc[0], whc[1], whc[2]
    out = np.zeros((h, w, c), np.uint8)
    rc = lib.smvs_host_load_byte_image(path.encode(), whc, out.ctypes.data_as(_u8p),
                                       C.c_size_t(out.size))
    if rc != 0:
        raise _capi.SmvsError(rc, lib.smvs_host_last_error().decode())
    return out if c > 1 else out.reshape(h, w)


def shading_planes(img, gamma=False):
    """The host's StereoView::initialize_linear (lib/stereo_view.cc:64-84) of a
    view with the u8 image `img` (h, w) or (h, w, c): (shading (h, w), shading
    gradients (h, w, 2)).  Needs no device."""
    lib = load()
    a = np.ascontiguousarray(img, dtype=np.uint8)
    if a.ndim == 2:
        a = a[:, :, None]
    h, w, c = a.shape
    shading = np.zeros((h, w), np.float32)
    grad = np.zeros((h, w, 2), np.float32)
    rc = lib.smvs_host_shading_planes(a.ctypes.data_as(_u8p), C.c_int(w), C.c_int(h),
                                      C.c_int(c), C.c_int(1 if gamma else 0),
                                      shading.ctypes.data_as(_fp), grad.ctypes.data_as(_fp))
    if rc != 0:
        raise _capi.SmvsError(rc, lib.smvs_host_last_error().decode())
    return shading, grad


def gamma_inv_srgb_lut():
    """imgtools::gamma_inv_srgb_lut: the inverse sRGB curve of
    initialize_linear at the 256 values np.float32(k) / 255 an image element
    can take -- the table smvs_ctx_prepare_shading looks up."""
    lib = load()
    lut = np.zeros(256, np.float32)
    rc = lib.smvs_host_gamma_inv_srgb_lut(lut.ctypes.data_as(_fp))
    if rc != 0:
        raise _capi.SmvsError(rc, lib.smvs_host_last_error().decode())
    return lut


def save_png(path, array):
    lib = load()
    a = np.ascontiguousarray(array, dtype=np.uint8)
    if a.ndim == 2:
        a = a[:, :, None]
    rc = lib.smvs_host_save_png(path.encode(), a.ctypes.data_as(_u8p), C.c_int(a.shape[1]),
                                C.c_int(a.shape[0]), C.c_int(a.shape[2]))
    if rc != 0:
        raise _capi.SmvsError(rc, lib.smvs_host_last_error().decode())


def rescale_half_size_gaussian(array, halvings=1, device=None):
    """mve::image::rescale_half_size_gaussian<uint8_t> of the host mirror,
    `halvings` times.  device=None: the host loop; device=k: the whole chain on
    device k (rescale_half_size_gaussian_device), the same bytes."""
    lib = load()
    a = np.ascontiguousarray(array, dtype=np.uint8)
    squeeze = a.ndim == 2
    if squeeze:
        a = a[:, :, None]
    if device is None:
        if halvings < 1:
            raise ValueError("rescale_half_size_gaussian: halvings < 1")
        for _ in range(halvings):
            h, w, c = a.shape
            out = np.zeros(((h + 1) // 2, (w + 1) // 2, c), np.uint8)
            rc = lib.smvs_host_rescale_half_size_gaussian(a.ctypes.data_as(_u8p), C.c_int(w),
                                                          C.c_int(h), C.c_int(c),
                                                          out.ctypes.data_as(_u8p))
            if rc != 0:
                raise _capi.SmvsError(rc, lib.smvs_host_last_error().decode())
            a = out
    else:
        h, w, c = a.shape
        ow, oh = w, h
        for _ in range(max(halvings, 0)):
            ow, oh = (ow + 1) // 2, (oh + 1) // 2
        out = np.zeros((oh, ow, c), np.uint8)
        gw, gh = C.c_int(0), C.c_int(0)
        rc = lib.smvs_host_rescale_half_size_gaussian_device(
            a.ctypes.data_as(_u8p), C.c_int(w), C.c_int(h), C.c_int(c), C.c_int(halvings),
            C.c_int(device), out.ctypes.data_as(_u8p), C.c_size_t(out.size), C.byref(gw),
            C.byref(gh))
        if rc != 0:
            raise _capi.SmvsError(rc, lib.smvs_host_last_error().decode())
        assert (gw.value, gh.value) == (ow, oh)
    return out[:, :, 0] if squeeze else out


def scene_info(scene_dir, image_embedding="undistorted", max_views=4096):
    """Scene::create + bundle of csrc/host/scene_io.cc (no device)."""
    lib = load()
    n = C.c_int(0); nf = C.c_int(0)
    present = np.zeros(max_views, np.int32); flen = np.zeros(max_views, np.float32)
    rot = np.zeros((max_views, 9), np.float32); trans = np.zeros((max_views, 3), np.float32)
    w = np.zeros(max_views, np.int32); h = np.zeros(max_views, np.int32)
    rc = lib.smvs_host_scene_info(scene_dir.encode(), image_embedding.encode(),
        C.c_int(max_views), C.byref(n), present.ctypes.data_as(_i32p),
        flen.ctypes.data_as(_fp), rot.ctypes.data_as(_fp), trans.ctypes.data_as(_fp),
        w.ctypes.data_as(_i32p), h.ctypes.data_as(_i32p), C.byref(nf))
    if rc != 0:
        raise _capi.SmvsError(rc, lib.smvs_host_last_error().decode())
    k = n.value
    return dict(present=present[:k], flen=flen[:k], rot=rot[:k], trans=trans[:k],
                width=w[:k], height=h[:k], n_features=nf.value)


def mvei_roundtrip(in_path, out_path):
    lib = load()
    if lib.smvs_host_mvei_roundtrip(in_path.encode(), out_path.encode()) != 0:
        raise _capi.SmvsError(-1, lib.smvs_host_last_error().decode())


def view_queue_selftest(n_tasks, num_devices, views_in_flight, throwing_task=-1):
    """smvs_amd::ViewQueue without a device: -> (tasks per device, per worker)."""
    lib = load()
    dev = np.zeros(num_devices, np.int32)
    wrk = np.zeros(num_devices * views_in_flight, np.int32)
    rc = lib.smvs_host_view_queue_selftest(C.c_int(n_tasks), C.c_int(num_devices),
        C.c_int(views_in_flight), C.c_int(throwing_task), dev.ctypes.data_as(_i32p),
        wrk.ctypes.data_as(_i32p))
    if rc != 0:
        raise _capi.SmvsError(rc, lib.smvs_host_last_error().decode())
    return dev, wrk


def sgm_depth(inputs, sgm_scale=1, min_depth=0.0, max_depth=0.0, device=0,
              adaptive_penalty2=False, num_steps=128, subplane=False, neighbors=2,
              consensus=False, agree_ratio=0.95, min_agree=2, sweep=False,
              sweep_min_views=-1, sweep_best_k=-1, sweep_support_cost=20,
              sweep_min_support=-1, uniqueness=0, uniqueness_window=1, speckle_size=0,
              speckle_ratio=0.95, photo_radius=0, photo_best_k=2, photo_min_views=2,
              photo_min_score=0.49, photo_witnesses=-1, refine_sweeps=0, refine_samples=2,
              refine_depth_step=0.02, refine_slant_step=0.01, refine_seed=1, refine_fill=1):
    """reconstruct_sgm_depth_for_view through the host mirror.
    adaptive_penalty2: SGMStereo::Options::adaptive_penalty2 (the reference's
    build without SSE, lib/sgm_stereo.cc:310-346); off by default.
    num_steps: SGMStereo::Options::num_steps, the inverse-depth planes: 2 .. 128,
    or a multiple of 8 from 136 to 256.
    subplane: SGMStereo::Options::subplane (the winning plane's depth refined by
    the parabola through its aggregated cost and its two neighbours'; not in
    the reference); off by default.
    neighbors, consensus, agree_ratio, min_agree: SGMStereo::Options::
    num_neighbors / consensus / agree_ratio / min_agree -- the first `neighbors`
    neighbours of the inputs, merged by consensus (SMVS_SGM_MERGE_CONSENSUS of
    include/smvs_hip.h: per pixel the mean of the largest group of checked
    depths whose ratio to one of them is at least agree_ratio, none with fewer
    than min_agree).  More than two neighbours without consensus raise; off by
    default.  0.95 and 2 are defaults of a user option, not tuned values (0.95
    admits about two of 128 planes at the far end of a 3 .. 12 range; the
    left/right check uses 0.8); nobody has measured their effect on real scenes.
    sweep and its four values: SGMStereo::Options::sweep / ... -- the
    multi-neighbour plane sweep of include/smvs_hip.h over the first `neighbors`
    neighbours instead of the runs and the merge; raises together with
    consensus.  -1: the default at n neighbours (min_views min(2, n), best_k
    (n + 1) // 2, min_support min(2, n)); untuned defaults of a user option,
    nobody has measured them on real scenes.  Off by default.
    uniqueness, uniqueness_window, speckle_size, speckle_ratio:
    SGMStereo::Options::uniqueness / ... -- the two filters of include/smvs_hip.h
    for any of the three front ends (the uniqueness test in every run, the
    speckle removal on the final map); off by default, (0, 1, 0, 0.95) are
    untuned defaults of a user option.
    photo_radius, photo_best_k, photo_min_views, photo_min_score, photo_witnesses:
    SGMStereo::Options::photo_radius / ... -- the multi-view photo-consistency
    test of include/smvs_hip.h on the final map of any of the three front ends,
    before the speckle removal, with the first photo_witnesses neighbours of the
    inputs as witnesses (-1: all of them, 16 at the most).  With photo_radius
    > 0 returns (depth, confidence), the confidence being what the mirror writes
    as the smvs-sgm-confidence embedding.  Off by default; (0, 2, 2, 0.49, -1)
    are untuned defaults of a user option.
    refine_sweeps, refine_samples, refine_depth_step, refine_slant_step,
    refine_seed, refine_fill: SGMStereo::Options::refine_sweeps / ... -- the
    multi-view plane refinement sweeps of include/smvs_hip.h in the photo test's
    place (they need photo_radius > 0).  With refine_sweeps > 0 returns (depth,
    confidence, slant), the slant (h, w, 2) being what the mirror writes as the
    smvs-sgm-slant embedding.  Off by default; (0, 2, 0.02, 0.01, 1, 1) are
    untuned defaults of a user option."""
    lib = load()
    keep = []
    refine = SgmRefine(int(refine_sweeps), int(refine_samples), float(refine_depth_step),
                       float(refine_slant_step), int(refine_seed) & 0xFFFFFFFF,
                       int(refine_fill))
    photo = SgmPhoto(int(photo_radius), int(photo_best_k), int(photo_min_views),
                     float(photo_min_score), int(photo_witnesses))
    filt = SgmFilter(int(uniqueness), int(uniqueness_window), int(speckle_size),
                     float(speckle_ratio))
    sw = SgmSweep(1 if sweep else 0, sweep_min_views, sweep_best_k, sweep_support_cost,
                  sweep_min_support)
    main, subs, n_subs, b = _marshal(inputs, keep)
    w, h = main.width, main.height
    for _ in range(sgm_scale):
        w, h = (w + 1) // 2, (h + 1) // 2
    out = np.zeros((h, w), dtype=np.float32)
    conf = np.zeros((h, w), dtype=np.float32) if photo.radius != 0 else None
    slant = np.zeros((h, w, 2), dtype=np.float32) if refine.sweeps != 0 else None
    ow = C.c_int(0); oh = C.c_int(0)
    rc = lib.smvs_host_sgm_depth_refine(C.byref(main), subs, n_subs, C.byref(b),
        sgm_scale, C.c_float(min_depth), C.c_float(max_depth), device,
        C.c_int(1 if adaptive_penalty2 else 0), C.c_int(num_steps),
        C.c_int(1 if subplane else 0), C.c_int(neighbors), C.c_int(1 if consensus else 0),
        C.c_float(agree_ratio), C.c_int(min_agree), C.byref(sw), C.byref(filt),
        C.byref(photo), C.byref(refine), out.ctypes.data_as(_fp),
        conf.ctypes.data_as(_fp) if conf is not None else None,
        slant.ctypes.data_as(_fp) if slant is not None else None, C.byref(ow), C.byref(oh))
    if rc != 0:
        raise _capi.SmvsError(rc, lib.smvs_host_last_error().decode())
    assert (ow.value, oh.value) == (w, h)
    if slant is not None:
        return out, conf, slant
    return out if conf is None else (out, conf)


def select_neighbors(scene, view, num_neighbors=6, use_bundle=True):
    """smvs_amd::ViewSelection (csrc/host/view_selection.cc, mirror of
    lib/view_selection.cc:14-161) on a scene description: dict(views=[dict(
    present, id, flen, rot, trans, has_image, width, height)], features=(F, 3),
    refs=[view ids per feature]).  Returns indices into the view list."""
    lib = load()
    keep = []
    n = len(scene["views"])
    views = (HostView * n)()
    dummy = np.zeros(1, dtype=np.uint8)
    for i, v in enumerate(scene["views"]):
        present = v.get("present", True)
        views[i].width = int(v["width"]) if present else 0
        views[i].height = int(v["height"]) if present else 0
        views[i].channels = 1
        views[i].bytes = dummy.ctypes.data_as(_u8p) if v.get("has_image", True) else None
        views[i].flen = float(v["flen"])
        for k, x in enumerate(np.asarray(v["rot"], dtype=np.float32).reshape(9)):
            views[i].rot[k] = float(x)
        for k, x in enumerate(np.asarray(v["trans"], dtype=np.float32).reshape(3)):
            views[i].trans[k] = float(x)
        views[i].view_id = int(v["id"])
    bundle = None
    if use_bundle:
        feats = np.ascontiguousarray(scene["features"], dtype=np.float32).reshape(-1, 3)
        offsets = np.zeros(len(scene["refs"]) + 1, dtype=np.int32)
        offsets[1:] = np.cumsum([len(r) for r in scene["refs"]])
        flat = np.asarray([i for r in scene["refs"] for i in r], dtype=np.int32)
        if flat.size == 0:
            flat = np.zeros(1, dtype=np.int32)
        keep += [feats, offsets, flat]
        bundle = HostBundle(feats.shape[0], feats.ctypes.data_as(_fp),
                            offsets.ctypes.data_as(_i32p), flat.ctypes.data_as(_i32p))
    out = np.zeros(max(n, 1), dtype=np.int32)
    n_out = C.c_int(0)
    rc = lib.smvs_host_select_neighbors(views, C.c_int(n),
        C.byref(bundle) if bundle is not None else None, C.c_int(view),
        C.c_int(num_neighbors), out.ctypes.data_as(_i32p), C.byref(n_out))
    if rc != 0:
        raise _capi.SmvsError(rc, lib.smvs_host_last_error().decode())
    return [int(x) for x in out[:n_out.value]]


def slant_plane(lowres, slants, width, height):
    """Surface::slant_plane, the tap rule of smvs_ctx_sgm_init_slants on the host
    (no device involved): the SGM-scale z-depth map and its (h, w, 2) slants ->
    the (height, width, 2) plane."""
    lib = load()
    lo = np.ascontiguousarray(lowres, dtype=np.float32)
    sl = np.ascontiguousarray(slants, dtype=np.float32)
    if sl.shape != lo.shape + (2,):
        raise ValueError("slants must be lowres.shape + (2,)")
    out = np.zeros((height, width, 2), np.float32)
    rc = lib.smvs_host_slant_plane(lo.ctypes.data_as(_fp), sl.ctypes.data_as(_fp),
        C.c_int(lo.shape[1]), C.c_int(lo.shape[0]), C.c_int(width), C.c_int(height),
        out.ctypes.data_as(_fp))
    if rc != 0:
        raise _capi.SmvsError(rc, lib.smvs_host_last_error().decode())
    return out


def surface_script(inputs, init_scale, ops, init_depth=None, delete_every=3, device=None,
                   init_slant=None):
    """smvs_amd::Surface on its own (csrc/host/surface.cc, mirror of
    lib/surface.cc): create + a script of operations (1 expand,
    2 subdivide_patches, 3 fill_patches_from_depth, 4 remove_isolated_patches,
    5 delete every delete_every-th valid patch + remove_nodes_without_patch).
    device=None: the host mirror, no device involved; device=k: the same
    script on the surface of a device context (csrc/surface.hip), result
    downloaded (plus valid_patches as the last operation reported it).
    init_slant (with init_depth): the (H, W, 2) slant plane the node slopes come
    from (Surface::create(..., init, slant) / smvs_surface_create_planes)."""
    lib = load()
    keep = []
    main, _, _, bundle = _marshal(inputs, keep)
    h, w = np.asarray(inputs["images"][0]).shape[:2]
    cap_n, cap_p = (w + 2) * (h + 2), (w + 1) * (h + 1)
    nodes = np.zeros(cap_n * 4); nv = np.zeros(cap_n, np.uint8); pv = np.zeros(cap_p, np.uint8)
    info = np.zeros(6, np.int32)
    ops_a = np.asarray(list(ops) + [0], dtype=np.int32)
    depth = None if init_depth is None else np.ascontiguousarray(init_depth, dtype=np.float32)
    dptr = depth.ctypes.data_as(_fp) if depth is not None else None
    if init_slant is not None:
        if depth is None:
            raise ValueError("init_slant needs init_depth")
        plane = np.ascontiguousarray(init_slant, dtype=np.float32)
        if plane.shape != (h, w, 2):
            raise ValueError("init_slant must be (H, W, 2)")
        tail = (info.ctypes.data_as(_i32p), nodes.ctypes.data_as(C.POINTER(C.c_double)),
                nv.ctypes.data_as(_u8p), pv.ctypes.data_as(_u8p))
        head = (C.byref(main), dptr, plane.ctypes.data_as(_fp), C.c_int(init_scale),
                ops_a.ctypes.data_as(_i32p), C.c_int(len(ops)), C.c_int(delete_every))
        if device is None:
            rc = lib.smvs_host_surface_script_planes(*head, *tail)
        else:
            rc = lib.smvs_host_surface_script_planes_device(*head, C.c_int(device), *tail)
    elif device is None:
        rc = lib.smvs_host_surface_script(C.byref(main), C.byref(bundle), dptr,
            C.c_int(init_scale), ops_a.ctypes.data_as(_i32p), C.c_int(len(ops)),
            C.c_int(delete_every), info.ctypes.data_as(_i32p),
            nodes.ctypes.data_as(C.POINTER(C.c_double)), nv.ctypes.data_as(_u8p),
            pv.ctypes.data_as(_u8p))
    else:
        rc = lib.smvs_host_surface_script_device(C.byref(main), C.byref(bundle), dptr,
            C.c_int(init_scale), ops_a.ctypes.data_as(_i32p), C.c_int(len(ops)),
            C.c_int(delete_every), C.c_int(device), info.ctypes.data_as(_i32p),
            nodes.ctypes.data_as(C.POINTER(C.c_double)), nv.ctypes.data_as(_u8p),
            pv.ctypes.data_as(_u8p))
    if rc != 0:
        raise _capi.SmvsError(rc, lib.smvs_host_last_error().decode())
    scale, npx, npy, sx, sy = (int(x) for x in info[:5])
    nn, npatch = (npx + 1) * (npy + 1), npx * npy
    out = dict(scale=scale, npx=npx, npy=npy, start_x=sx, start_y=sy,
               nodes=nodes[:4 * nn].reshape(nn, 4).copy(), node_valid=nv[:nn].copy(),
               patch_valid=pv[:npatch].copy())
    if device is not None:
        out["valid_patches"] = int(info[5])
    return out


def surface_maps(inputs, init_scale, init_depth=None, device=0, init_slant=None):
    """DepthOptimizer(main, subs, surface, opts).get_depth() / get_normals()
    without optimize() (lib/depth_optimizer.h:53-61).  init_slant (with
    init_depth): the (H, W, 2) slant plane of Surface::create.  device=None (with
    init_depth): the host mirror's Surface::get_depth_map / get_normal_map, no
    device involved."""
    lib = load()
    keep = []
    main, subs, n_subs, b = _marshal(inputs, keep)
    h, w = main.height, main.width
    depth = np.zeros((h, w), dtype=np.float32)
    normals = np.zeros((h, w, 3), dtype=np.float32)
    init = None if init_depth is None else np.ascontiguousarray(init_depth, dtype=np.float32)
    if init_slant is not None or device is None:
        if init is None:
            raise ValueError("init_slant / device=None need init_depth")
        plane = None
        if init_slant is not None:
            plane = np.ascontiguousarray(init_slant, dtype=np.float32)
            if plane.shape != (h, w, 2):
                raise ValueError("init_slant must be (H, W, 2)")
        pptr = plane.ctypes.data_as(_fp) if plane is not None else None
        if device is None:
            rc = lib.smvs_host_surface_maps_host(C.byref(main), init.ctypes.data_as(_fp), pptr,
                C.c_int(init_scale), depth.ctypes.data_as(_fp), normals.ctypes.data_as(_fp))
        else:
            rc = lib.smvs_host_surface_maps_planes(C.byref(main), subs, n_subs, C.byref(b),
                init.ctypes.data_as(_fp), pptr, C.c_int(init_scale), C.c_int(device),
                depth.ctypes.data_as(_fp), normals.ctypes.data_as(_fp))
        if rc != 0:
            raise _capi.SmvsError(rc, lib.smvs_host_last_error().decode())
        return depth, normals
    rc = lib.smvs_host_surface_maps(C.byref(main), subs, n_subs, C.byref(b),
        init.ctypes.data_as(_fp) if init is not None else None, C.c_int(init_scale),
        C.c_int(device), depth.ctypes.data_as(_fp), normals.ctypes.data_as(_fp))
    if rc != 0:
        raise _capi.SmvsError(rc, lib.smvs_host_last_error().decode())
    return depth, normals


def depth_range(inputs, view_index=0):
    """SGMStereo::fill_depth_range_for_view on the host mirror."""
    lib = load()
    keep = []
    _, _, _, bundle = _marshal(inputs, keep)
    v = _view(inputs["images"][view_index], inputs["cams"][view_index],
              inputs["view_ids"][view_index], keep)
    out = np.zeros(2, np.float32)
    if lib.smvs_host_depth_range(C.byref(v), C.byref(bundle), out.ctypes.data_as(_fp)) != 0:
        raise _capi.SmvsError(-1, lib.smvs_host_last_error().decode())
    return out


def view_reprojection(inputs, src, dst):
    """CameraInfo::fill_reprojection between two views at their image sizes."""
    lib = load()
    keep = []
    a = _view(inputs["images"][src], inputs["cams"][src], inputs["view_ids"][src], keep)
    b = _view(inputs["images"][dst], inputs["cams"][dst], inputs["view_ids"][dst], keep)
    M = np.zeros(9, np.float32); t = np.zeros(3, np.float32)
    if lib.smvs_host_reprojection(C.byref(a), C.byref(b), M.ctypes.data_as(_fp),
                                  t.ctypes.data_as(_fp)) != 0:
        raise _capi.SmvsError(-1, lib.smvs_host_last_error().decode())
    return M, t


def sgm_image(inputs, view_index=0, halvings=1):
    """StereoView::get_byte_image + rescale_half_size (the SGM input image)."""
    lib = load()
    keep = []
    v = _view(inputs["images"][view_index], inputs["cams"][view_index],
              inputs["view_ids"][view_index], keep)
    out = np.zeros(v.width * v.height, np.uint8)
    w, h = C.c_int(0), C.c_int(0)
    if lib.smvs_host_sgm_image(C.byref(v), C.c_int(halvings), out.ctypes.data_as(_u8p),
                               C.byref(w), C.byref(h)) != 0:
        raise _capi.SmvsError(-1, lib.smvs_host_last_error().decode())
    return out[:w.value * h.value].reshape(h.value, w.value).copy()


def block_multiply(H9, node_stride, x):
    """smvs_amd::BlockStencilMatrix::multiply (BlockSparseMatrix<4>::multiply,
    lib/block_sparse_matrix.h:276-298) on the host: y = A x for the block
    stencil H9 [N][9][16].  No device involved."""
    lib = load()
    H9 = np.ascontiguousarray(H9, dtype=np.float64)
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
    n = x.size // 4
    y = np.zeros(4 * n)
    dp = C.POINTER(C.c_double)
    rc = lib.smvs_host_block_multiply(C.c_int(n), C.c_int(node_stride),
                                      H9.ctypes.data_as(dp), x.ctypes.data_as(dp),
                                      y.ctypes.data_as(dp))
    if rc != 0:
        raise _capi.SmvsError(rc, lib.smvs_host_last_error().decode())
    return y


# ------------------------------------------------------------ loop recording
def record_loops(on=True):
    """smvs_host_record_loops: while on, every Newton batch of this thread's
    optimize() calls leaves a device-resident clone of its loop's start state
    (smvs_ctx_clone_loop_state); starting a recording drops what the recorder
    still owns."""
    load().smvs_host_record_loops(1 if on else 0)


def take_recorded_loops():
    """-> [dict(handle, params, scale, iter)] of this thread's recording; the
    contexts now belong to the caller (smvs_ctx_destroy each)."""
    lib = load()
    n = lib.smvs_host_recorded_loops(None, None, None, None, 0)
    if n == 0:
        return []
    ctxs = (C.c_void_p * n)()
    prm = (_capi.LoopParams * n)()
    scales = (C.c_int * n)()
    iters = (C.c_int * n)()
    lib.smvs_host_recorded_loops(ctxs, prm, scales, iters, n)
    lib.smvs_host_release_recorded_loops(0)
    return [dict(handle=C.c_void_p(ctxs[i]), params=prm[i], scale=scales[i], iter=iters[i])
            for i in range(n)]


# ---------------------------------------------------------------- embeddings
def last_embeddings():
    """{name: array} of what the last optimize() of this thread wrote into its
    main view (smvs_host_embedding_names / smvs_host_embedding): the results and,
    with SMVS_DEBUG_LVL >= 2, the reference's intermediate embeddings."""
    lib = load()
    buf = C.create_string_buffer(4096)
    lib.smvs_host_embedding_names(buf, 4096)
    out = {}
    for name in buf.value.decode().split("\n"):
        if not name:
            continue
        whc = (C.c_int * 3)()
        n = lib.smvs_host_embedding(name.encode(), None, C.c_longlong(0), whc)
        if n <= 0:
            continue
        a = np.zeros(n, dtype=np.float32)
        if lib.smvs_host_embedding(name.encode(), a.ctypes.data_as(_fp), C.c_longlong(n), whc) == 0:
            out[name] = a.reshape(whc[1], whc[0], whc[2]).squeeze()
    return out


class PointCloudSettings(C.Structure):
    _fields_ = [("image_embedding", C.c_char_p), ("input_scale", C.c_int),
                ("use_shading", C.c_int), ("cut_surface", C.c_int),
                ("create_triangle_mesh", C.c_int), ("simplify", C.c_int),
                ("use_aabb", C.c_int), ("aabb_min", C.c_float * 3),
                ("aabb_max", C.c_float * 3), ("device", C.c_int)]


def _point_cloud_settings(image_embedding, input_scale, use_shading, cut, aabb, mesh,
                          simplify, device):
    st = PointCloudSettings()
    st.image_embedding = image_embedding.encode()
    st.input_scale = int(input_scale)
    st.use_shading = int(bool(use_shading))
    st.cut_surface = int(bool(cut))
    st.create_triangle_mesh = int(bool(mesh))
    st.simplify = int(bool(simplify))
    st.use_aabb = int(aabb is not None)
    if aabb is not None:
        for k in range(3):
            st.aabb_min[k] = float(aabb[0][k])
            st.aabb_max[k] = float(aabb[1][k])
    st.device = int(device)
    return st


def generate_point_cloud(scene_dir, view_ids=None, image_embedding="undistorted",
                         input_scale=0, use_shading=False, cut=True, aabb=None,
                         mesh=False, simplify=False, device=0):
    """smvsrecon's generate_mesh (app/smvsrecon.cc:278-343) on a reconstructed
    scene through smvs_amd::generate_scene_point_cloud: the point cloud of the
    views' smvs-{B,S}<input_scale> embeddings, written as
    <scene>/smvs-{B,S}<input_scale>.ply (and smvs-cut.mvei per view when
    cutting).  aabb: None or (min3, max3).  mesh / simplify (--mesh,
    --simplify) are refused (the mesh: generate_mesh).  Returns (ply path,
    number of points)."""
    lib = load()
    st = _point_cloud_settings(image_embedding, input_scale, use_shading, cut, aabb, mesh,
                               simplify, device)
    ids = None if view_ids is None else np.asarray(view_ids, dtype=np.int32)
    path = C.create_string_buffer(4096)
    n = C.c_int64(0)
    rc = lib.smvs_host_generate_point_cloud(
        scene_dir.encode(), C.byref(st), ids.ctypes.data_as(_i32p) if ids is not None else None,
        C.c_int(0 if ids is None else ids.size), path, C.c_int(len(path)), C.byref(n))
    if rc != 0:
        raise _capi.SmvsError(rc, lib.smvs_host_last_error().decode())
    return path.value.decode(), n.value


def generate_mesh(scene_dir, view_ids=None, image_embedding="undistorted", input_scale=0,
                  use_shading=False, cut=True, aabb=None, simplify=False, device=0):
    """smvsrecon --mesh on a reconstructed scene through
    smvs_amd::generate_scene_mesh: the triangle mesh of the views'
    smvs-{B,S}<input_scale> embeddings, written as
    <scene>/smvs-m-{B,S}<input_scale>.ply (and smvs-cut.mvei per view when
    cutting).  aabb: None or (min3, max3); simplify (--simplify) is refused.
    Returns (ply path, number of vertices, number of faces)."""
    lib = load()
    st = _point_cloud_settings(image_embedding, input_scale, use_shading, cut, aabb, True,
                               simplify, device)
    ids = None if view_ids is None else np.asarray(view_ids, dtype=np.int32)
    path = C.create_string_buffer(4096)
    nv, nf = C.c_int64(0), C.c_int64(0)
    rc = lib.smvs_host_generate_mesh(
        scene_dir.encode(), C.byref(st), ids.ctypes.data_as(_i32p) if ids is not None else None,
        C.c_int(0 if ids is None else ids.size), path, C.c_int(len(path)), C.byref(nv),
        C.byref(nf))
    if rc != 0:
        raise _capi.SmvsError(rc, lib.smvs_host_last_error().decode())
    return path.value.decode(), nv.value, nf.value


def generate_simplified(scene_dir, mesh=False, view_ids=None, image_embedding="undistorted",
                        input_scale=0, use_shading=False, cut=True, aabb=None, device=0):
    """smvsrecon --simplify (mesh=True: --mesh --simplify) on a reconstructed
    scene through smvs_amd::generate_scene_simplified: every view's greedy
    Delaunay triangulation, written under the
    reference's names <scene>/smvs-{B,S}<input_scale>.ply or, with the mesh,
    smvs-m-{B,S}<input_scale>.ply (and smvs-cut.mvei per view when cutting).
    Returns (ply path, number of vertices, number of faces; 0 faces for the
    point cloud)."""
    lib = load()
    st = _point_cloud_settings(image_embedding, input_scale, use_shading, cut, aabb, mesh,
                               True, device)
    ids = None if view_ids is None else np.asarray(view_ids, dtype=np.int32)
    path = C.create_string_buffer(4096)
    nv, nf = C.c_int64(0), C.c_int64(0)
    rc = lib.smvs_host_generate_simplified(
        scene_dir.encode(), C.byref(st), ids.ctypes.data_as(_i32p) if ids is not None else None,
        C.c_int(0 if ids is None else ids.size), path, C.c_int(len(path)), C.byref(nv),
        C.byref(nf))
    if rc != 0:
        raise _capi.SmvsError(rc, lib.smvs_host_last_error().decode())
    return path.value.decode(), nv.value, nf.value


class FusedSettings(C.Structure):
    _fields_ = [("voxel_size", C.c_float), ("resolution", C.c_int), ("trunc", C.c_float),
                ("min_weight", C.c_int)]


class FusedSparseSettings(C.Structure):
    _fields_ = [("voxel_size", C.c_float), ("resolution", C.c_int), ("trunc", C.c_float),
                ("min_weight", C.c_int), ("max_bricks", C.c_int64)]


class FusedSparseCullSettings(C.Structure):
    _fields_ = FusedSparseSettings._fields_ + [("cull", C.c_int)]


class FusedCleanSettings(C.Structure):
    """smvs_host_fused_clean_settings"""
    _fields_ = FusedSparseCullSettings._fields_ + [
        ("sparse", C.c_int), ("threshold", C.c_float), ("percentile", C.c_float),
        ("component_size", C.c_int), ("keep_unreferenced", C.c_int)]


class FusedBatchedSettings(C.Structure):
    """smvs_host_fused_batched_settings"""
    _fields_ = FusedCleanSettings._fields_ + [("clean", C.c_int), ("batch_views", C.c_int)]


class FusedSparseBatchedSettings(C.Structure):
    """smvs_host_fused_sparse_batched_settings"""
    _fields_ = FusedBatchedSettings._fields_ + [("sparse_batch_views", C.c_int)]


# generate_fused: the record, the entry and whether it takes the clean's stats;
# every record is the widest one cut to its field count
_FUSED_ENTRIES = {
    "dense": (FusedSettings, "smvs_host_generate_fused", False),
    "sparse": (FusedSparseSettings, "smvs_host_generate_fused_sparse", False),
    "sparse_cull": (FusedSparseCullSettings, "smvs_host_generate_fused_sparse_cull", False),
    "clean": (FusedCleanSettings, "smvs_host_generate_fused_clean", True),
    "batched": (FusedBatchedSettings, "smvs_host_generate_fused_batched", True),
    "sparse_batched": (FusedSparseBatchedSettings, "smvs_host_generate_fused_sparse_batched",
                       True),
}
# smvs_amd.clean_mesh's defaults
_CLEAN_DEFAULTS = dict(threshold=0.0, percentile=0.0, component_size=1000,
                       keep_unreferenced=False)


def generate_fused(scene_dir, voxel_size=None, resolution=256, aabb=None, trunc=0, min_weight=0,
                   view_ids=None, image_embedding="undistorted", input_scale=0,
                   use_shading=False, cut=True, device=0, sparse=False, max_bricks=0,
                   cull=False, clean=None, batch_views=0, sparse_batch_views=0):
    """Not in the reference: the views' smvs-{B,S}<input_scale> depth maps fused
    into ONE surface mesh through a truncated signed distance field
    (smvs_tsdf_fuse), written as
    <scene>/smvs-fused-{B,S}<input_scale>.ply.  The box is aabb ((min3, max3)),
    or the bounds of the (cut) depth maps' points padded by the truncation
    distance; voxel_size None: the box's longest side / resolution; trunc 0: 3
    voxels; min_weight 0: 1.  Returns (ply path, number of vertices, number of
    faces).

    sparse: the volume is allocated in 8 x 8 x 4 bricks near the surface
    (smvs_tsdf_fuse_sparse, section 9.9): the same mesh with vertices and faces
    in the brick order, under the same file name; resolution may go up to 4096;
    max_bricks 0: 1 << 20 bricks.  cull (with sparse): the brick cull against
    the views' depth min/max pyramids in front of the seed pass (section 9.10);
    the file is the same byte for byte.

    clean: None, or dict(threshold=, percentile=, component_size=,
    keep_unreferenced=) -- smvs_amd.clean_mesh's options, the same defaults --
    and the fused mesh goes through smvs_mesh_clean_handle (section 9.12, what
    `meshclean -p10` does after fssrecon: percentile=10).  The cleaned mesh is
    written as <scene>/smvs-clean-{B,S}<input_scale>.ply, the fused file is
    not, and the call returns (ply path, number of vertices, number of faces,
    the clean's counts as clean_mesh's stats).

    batch_views: N > 0 keeps only N consecutive scene views loaded at a time
    (smvs_host_generate_fused_batched, section 9.13): the bounds are folded
    batch by batch, the batches are integrated into a persistent dense volume
    (smvs_amd.TsdfVolume) and the surface is extracted once.  With cut=False
    the file is the same byte for byte; the cut, when on, acts within a batch.
    It belongs to the dense volume: with sparse it is refused.  0: off.

    sparse_batch_views (with sparse): N > 0 keeps only N consecutive scene views
    loaded at a time on the brick-sparse volume
    (smvs_host_generate_fused_sparse_batched, section 9.14).  Three passes over
    the scene: the bounds (skipped with aabb), the marks (cull: with the brick
    cull in front) and the integration without growth into a persistent
    brick-sparse volume (smvs_amd.SparseTsdfVolume); then the surface is
    extracted once.  With cut=False the file is the same byte for byte; the
    cut, when on, acts within a batch.  0: off."""
    if sparse_batch_views and not sparse:
        raise ValueError("sparse_batch_views belongs to sparse=True")
    if cull and not sparse:
        raise ValueError("cull belongs to sparse=True")
    lib = load()
    st = _point_cloud_settings(image_embedding, input_scale, use_shading, cut, aabb, True,
                               False, device)
    if clean is not None:
        unknown = set(clean) - set(_CLEAN_DEFAULTS)
        if unknown:
            raise ValueError("clean: unknown option %s" % sorted(unknown))
    if max_bricks and not sparse:
        raise ValueError("max_bricks belongs to sparse=True")
    # the narrowest entry that states the request: it decides the error text
    key = ("sparse_batched" if sparse_batch_views else "batched" if batch_views
           else "clean" if clean is not None else "sparse_cull" if sparse and cull
           else "sparse" if sparse else "dense")
    record, name, takes_stats = _FUSED_ENTRIES[key]
    c = dict(_CLEAN_DEFAULTS, **(clean or {}))
    widest = (0.0 if voxel_size is None else float(voxel_size), int(resolution), float(trunc),
              int(min_weight), int(max_bricks), int(bool(cull)), int(bool(sparse)),
              float(c["threshold"]), float(c["percentile"]), int(c["component_size"]),
              int(bool(c["keep_unreferenced"])), int(clean is not None), int(batch_views),
              int(sparse_batch_views))
    fs = record(*widest[:len(record._fields_)])
    stats = _capi.MeshCleanStats() if clean is not None else None
    tail = (C.byref(stats) if stats is not None else None,) if takes_stats else ()
    ids = None if view_ids is None else np.asarray(view_ids, dtype=np.int32)
    path = C.create_string_buffer(4096)
    nv, nf = C.c_int64(0), C.c_int64(0)
    rc = getattr(lib, name)(
        scene_dir.encode(), C.byref(st), C.byref(fs),
        ids.ctypes.data_as(_i32p) if ids is not None else None,
        C.c_int(0 if ids is None else ids.size), path, C.c_int(len(path)), C.byref(nv),
        C.byref(nf), *tail)
    if rc != 0:
        raise _capi.SmvsError(rc, lib.smvs_host_last_error().decode())
    if stats is not None:
        return path.value.decode(), nv.value, nf.value, stats.as_dict()
    return path.value.decode(), nv.value, nf.value


def save_ply_points(path, xyz, normals, rgb, confidence, value):
    """The host's PLY writer of the point cloud (save_ply_points)."""
    lib = load()
    xyz = np.ascontiguousarray(xyz, np.float32)
    normals = np.ascontiguousarray(normals, np.float32)
    rgb = np.ascontiguousarray(rgb, np.uint8)
    confidence = np.ascontiguousarray(confidence, np.float32)
    value = np.ascontiguousarray(value, np.float32)
    n = confidence.size
    if xyz.shape != (n, 3) or normals.shape != (n, 3) or rgb.shape != (n, 3) \
            or value.size != n:
        raise ValueError("save_ply_points: attribute shapes differ")
    fp = C.POINTER(C.c_float)
    rc = lib.smvs_host_save_ply_points(
        path.encode(), xyz.ctypes.data_as(fp), normals.ctypes.data_as(fp),
        rgb.ctypes.data_as(C.POINTER(C.c_uint8)), confidence.ctypes.data_as(fp),
        value.ctypes.data_as(fp), C.c_int64(n))
    if rc != 0:
        raise _capi.SmvsError(rc, lib.smvs_host_last_error().decode())


def save_ply_mesh(path, xyz, normals, rgb, confidence, faces):
    """The host's PLY writer of the triangle mesh (save_ply_mesh)."""
    lib = load()
    xyz = np.ascontiguousarray(xyz, np.float32)
    normals = np.ascontiguousarray(normals, np.float32)
    rgb = np.ascontiguousarray(rgb, np.uint8)
    confidence = np.ascontiguousarray(confidence, np.float32)
    faces = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3)
    n = confidence.size
    if xyz.shape != (n, 3) or normals.shape != (n, 3) or rgb.shape != (n, 3):
        raise ValueError("save_ply_mesh: attribute shapes differ")
    fp = C.POINTER(C.c_float)
    rc = lib.smvs_host_save_ply_mesh(
        path.encode(), xyz.ctypes.data_as(fp), normals.ctypes.data_as(fp),
        rgb.ctypes.data_as(C.POINTER(C.c_uint8)), confidence.ctypes.data_as(fp),
        C.c_int64(n), faces.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_int64(len(faces)))
    if rc != 0:
        raise _capi.SmvsError(rc, lib.smvs_host_last_error().decode())


# ------------------------------------------------------------------ COLMAP
COLMAP_MODELS = {0: ("SIMPLE_PINHOLE", 3), 1: ("PINHOLE", 4), 2: ("SIMPLE_RADIAL", 4),
                 3: ("RADIAL", 5), 4: ("OPENCV", 8)}


class ImportSettings(C.Structure):
    """smvs_host_import_settings of csrc/host/host_capi.h."""
    _fields_ = [("device", C.c_int), ("zoom", C.c_float), ("out_width", C.c_int),
                ("out_height", C.c_int), ("container", C.c_int), ("threads", C.c_int),
                ("overwrite", C.c_int)]


class ImportReport(C.Structure):
    """smvs_host_import_report of csrc/host/host_capi.h."""
    _fields_ = [("num_views", C.c_int), ("views_written", C.c_int),
                ("points_kept", C.c_int64), ("points_dropped", C.c_int64),
                ("track_elements_kept", C.c_int64), ("track_elements_dropped", C.c_int64),
                ("seconds", C.c_double), ("decode_seconds", C.c_double),
                ("undistort_seconds", C.c_double), ("encode_seconds", C.c_double)]


def undistort(array, lens, out_focal, out_size=None, device=None, return_blank=False):
    """The undistortion resampling of include/smvs_hip.h (smvs_undistort_u8) of a
    u8 image (h, w) or (h, w, c): device=None is the host form
    (csrc/host/undistort_math.h, the kernel's own arithmetic), device=k the
    kernel on device k -- the same bytes.  lens: smvs_amd.device.make_lens;
    out_size = (width, height), the input's by default.  return_blank: (image,
    number of blank pixels)."""
    from .device import make_lens
    lib = load()
    a = np.ascontiguousarray(array, dtype=np.uint8)
    squeeze = a.ndim == 2
    if squeeze:
        a = a[:, :, None]
    h, w, c = a.shape
    ow, oh = (w, h) if out_size is None else (int(out_size[0]), int(out_size[1]))
    out = np.zeros((max(oh, 0), max(ow, 0), c), np.uint8)
    blank = C.c_int64(0)
    L = make_lens(lens)
    rc = lib.smvs_host_undistort_u8(a.ctypes.data_as(_u8p), C.c_int(w), C.c_int(h), C.c_int(c),
                                    C.byref(L), C.c_float(out_focal), C.c_int(ow), C.c_int(oh),
                                    C.c_int(-1 if device is None else device),
                                    out.ctypes.data_as(_u8p), C.byref(blank))
    if rc != 0:
        raise _capi.SmvsError(rc, lib.smvs_host_last_error().decode())
    out = out[:, :, 0] if squeeze else out
    return (out, blank.value) if return_blank else out


def _unpack_colmap(cams, imgs, pts):
    """The three sections of smvs_host_read_colmap_model (COLMAP's binary
    layout, tests/golden/COLMAP.md C6-C8) as dicts keyed by id."""
    import struct
    cameras, images, points = {}, {}, {}
    (n,), at = struct.unpack_from("<Q", cams, 0), 8
    for _ in range(n):
        cid, model, w, h = struct.unpack_from("<IiQQ", cams, at)
        at += 24
        name, k = COLMAP_MODELS[model]
        params = np.frombuffer(cams, "<f8", k, at).copy()
        at += 8 * k
        cameras[cid] = dict(model=name, width=w, height=h, params=params)
    (n,), at = struct.unpack_from("<Q", imgs, 0), 8
    for _ in range(n):
        iid = struct.unpack_from("<I", imgs, at)[0]
        q = np.frombuffer(imgs, "<f8", 4, at + 4).copy()
        t = np.frombuffer(imgs, "<f8", 3, at + 36).copy()
        cam = struct.unpack_from("<I", imgs, at + 60)[0]
        at += 64
        end = imgs.index(b"\0", at)
        name = imgs[at:end].decode()
        (m,), at = struct.unpack_from("<Q", imgs, end + 1), end + 9
        rec = np.frombuffer(imgs, np.dtype([("x", "<f8"), ("y", "<f8"), ("id", "<u8")]), m, at)
        at += 24 * m
        xys = np.stack([rec["x"], rec["y"]], axis=1) if m else np.zeros((0, 2))
        images[iid] = dict(q=q, t=t, camera_id=cam, name=name, xys=xys,
                           point3D_ids=rec["id"].astype(np.int64))
    (n,), at = struct.unpack_from("<Q", pts, 0), 8
    for _ in range(n):
        pid = struct.unpack_from("<Q", pts, at)[0]
        xyz = np.frombuffer(pts, "<f8", 3, at + 8).copy()
        rgb = np.frombuffer(pts, np.uint8, 3, at + 32).copy()
        err, m = struct.unpack_from("<dQ", pts, at + 35)
        at += 51
        track = np.frombuffer(pts, "<u4", 2 * m, at).reshape(m, 2).copy()
        at += 8 * m
        points[pid] = dict(xyz=xyz, rgb=rgb, error=err, image_ids=track[:, 0],
                           point2D_idxs=track[:, 1])
    return cameras, images, points


def read_colmap_model(model_dir):
    """read_colmap_model of csrc/host/colmap_io.cc: cameras / images / points3D of
    a COLMAP model (.bin if all three are there, else .txt), checked by the C++
    reader.  -> dict(binary, cameras={id: dict(model, width, height, params)},
    images={id: dict(q (w, x, y, z), t, camera_id, name, xys (m, 2), point3D_ids
    (m,), -1 for none)}, points3D={id: dict(xyz, rgb, error, image_ids,
    point2D_idxs)})."""
    lib = load()
    sizes = (C.c_uint64 * 3)()
    binary = C.c_int(0)
    rc = lib.smvs_host_read_colmap_model(model_dir.encode(), None, C.c_size_t(0), sizes,
                                         C.byref(binary))
    if rc != 0:
        raise _capi.SmvsError(rc, lib.smvs_host_last_error().decode())
    buf = np.zeros(max(sum(sizes), 1), np.uint8)
    rc = lib.smvs_host_read_colmap_model(model_dir.encode(), buf.ctypes.data_as(_u8p),
                                         C.c_size_t(buf.size), sizes, C.byref(binary))
    if rc != 0:
        raise _capi.SmvsError(rc, lib.smvs_host_last_error().decode())
    raw = buf.tobytes()
    a, b = sizes[0], sizes[0] + sizes[1]
    cameras, images, points = _unpack_colmap(raw[:a], raw[a:b], raw[b:b + sizes[2]])
    return dict(binary=bool(binary.value), cameras=cameras, images=images, points3D=points)


def import_colmap(model_dir, image_dir, scene_dir, zoom=1.0, device=None, out_size=None,
                  container="png", threads=4, view_ids=None, overwrite=False):
    """import_colmap of csrc/host/colmap_io.h: a COLMAP model and its images as
    the MVE scene `scene_dir` (views/view_%04d.mve/{meta.ini, undistorted.png},
    synth_0.out), every image resampled into a pinhole camera with a centred
    principal point and out_focal = zoom * fx -- by the host form (device=None)
    or by smvs_undistort_u8 on device k, the same bytes.  The images sorted by
    IMAGE_ID are the views 0 .. n - 1; view_ids restricts the views written.
    threads: host workers decode -> undistort -> encode, 1..16.  Returns the
    report as a dict; views[i]["blank_pixels"] counts the output pixels that see
    nothing of the source image (raise zoom to lose them)."""
    lib = load()
    if container not in ("png", "mvei"):
        raise ValueError("import_colmap: container must be 'png' or 'mvei'")
    ow, oh = (0, 0) if out_size is None else (int(out_size[0]), int(out_size[1]))
    st = ImportSettings(-1 if device is None else int(device), float(zoom), ow, oh,
                        0 if container == "png" else 1, int(threads), 1 if overwrite else 0)
    model = read_colmap_model(model_dir)
    names = {i: v["name"] for i, v in model["images"].items()}
    cap = max(len(names), 1)
    ids = None if view_ids is None else np.asarray(view_ids, dtype=np.int32)
    rep = ImportReport()
    vid = np.zeros(cap, np.int32); iid = np.zeros(cap, np.uint32)
    whc = np.zeros((cap, 3), np.int32); flen = np.zeros(cap, np.float32)
    blank = np.zeros(cap, np.int64)
    rc = lib.smvs_host_import_colmap(
        model_dir.encode(), image_dir.encode(), scene_dir.encode(), C.byref(st),
        ids.ctypes.data_as(_i32p) if ids is not None else None,
        C.c_int(0 if ids is None else ids.size), C.byref(rep), C.c_int(cap),
        vid.ctypes.data_as(_i32p), iid.ctypes.data_as(C.POINTER(C.c_uint32)),
        whc.ctypes.data_as(_i32p), flen.ctypes.data_as(_fp),
        blank.ctypes.data_as(C.POINTER(C.c_int64)))
    if rc != 0:
        raise _capi.SmvsError(rc, lib.smvs_host_last_error().decode())
    views = [dict(view_id=int(vid[i]), image_id=int(iid[i]), name=names[int(iid[i])],
                  width=int(whc[i, 0]), height=int(whc[i, 1]), channels=int(whc[i, 2]),
                  flen=float(flen[i]), blank_pixels=int(blank[i]))
             for i in range(min(rep.views_written, cap))]
    out = {k: getattr(rep, k) for k, _ in ImportReport._fields_}
    out["views"] = views
    return out
