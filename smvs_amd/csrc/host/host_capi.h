/* C entry points of the host mirror (libsmvs_host.so): lets tests / tools
 * drive smvs_amd::DepthOptimizer and smvs_amd::SGMStereo without a C++
 * toolchain.  Not part of the device boundary (that is include/smvs_hip.h). */
#ifndef SMVS_HOST_CAPI_H
#define SMVS_HOST_CAPI_H

#include <stddef.h>
#include <stdint.h>

#include "../../../include/smvs_hip.h"   /* smvs_lens */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int width, height, channels;
    const uint8_t *bytes;       /* interleaved u8 image */
    float flen;                 /* CameraInfo::flen */
    float rot[9], trans[3];
    int view_id;
} smvs_host_view;

typedef struct {
    int num_features;
    const float *positions;     /* num_features * 3 */
    const int *ref_offsets;     /* num_features + 1 */
    const int *ref_views;
} smvs_host_bundle;

typedef struct {                /* DepthOptimizer::Options */
    double regularization;
    double light_surf_regularization;
    int num_iterations;
    int min_scale;
    int use_shading;
    int use_sgm;
    int full_optimization;
    int device;
    int solver;                 /* smvs_solver_mode of include/smvs_hip.h */
    int gamma_correction;       /* StereoView::create's fourth argument for the main view
                                   (app/smvsrecon.cc:52, 669), with use_shading only */
} smvs_host_options;

#define SMVS_HOST_LOG_MAX 256
typedef struct {
    int count;
    int scale[SMVS_HOST_LOG_MAX];
    int iter[SMVS_HOST_LOG_MAX];
    int newton_steps[SMVS_HOST_LOG_MAX];
    int valid_patches[SMVS_HOST_LOG_MAX];
    int cg_iterations[SMVS_HOST_LOG_MAX];
    long long active_patch_steps[SMVS_HOST_LOG_MAX];   /* sum over the steps */
    double loop_seconds[SMVS_HOST_LOG_MAX];            /* device Newton loop */
    int has_lighting;
    double lighting[16];
} smvs_host_log;

const char *smvs_host_last_error(void);

/* DepthOptimizer(main, subs, bundle, opts).optimize().
 * sgm_depth: optional z-depth map (sgm_w x sgm_h) stored as the "smvs-sgm"
 * embedding; sgm_depth_roundtrip (optional, same size) receives what
 * StereoView::get_sgm_depth() hands to the optimizer. */
int smvs_host_optimize(const smvs_host_view *main_view,
    const smvs_host_view *subs, int n_subs, const smvs_host_bundle *bundle,
    const float *sgm_depth, int sgm_w, int sgm_h, float *sgm_depth_roundtrip,
    const smvs_host_options *opts, float *depth_out, float *normals_out,
    smvs_host_log *log);
/* The same with a word of switches smvs_host_options does not hold (it keeps
 * its layout for existing callers).  Bit 0: DepthOptimizer::Options::
 * device_shading_prep -- with use_shading, the main view's shading planes
 * (StereoView::initialize_linear, lib/stereo_view.cc:64-84) are made on the
 * device (smvs_ctx_prepare_shading) instead of on the host; the results are
 * the host path's, bit for bit.  An unknown bit is an argument error, raised
 * before anything else is looked at.  smvs_host_optimize forwards with 0. */
#define SMVS_HOST_OPTIMIZE_DEVICE_SHADING_PREP 1
/* Bit 1, known to smvs_host_optimize_planes only (to smvs_host_optimize_flags it
 * stays the unknown bit it was): DepthOptimizer::Options::init_slants -- the
 * initial surface's node slopes from the view's "smvs-sgm-slant" embedding.
 * Without use_sgm, or without a two-channel embedding of the size of
 * "smvs-sgm", an argument error before any device call. */
#define SMVS_HOST_OPTIMIZE_INIT_SLANTS 2
int smvs_host_optimize_flags(const smvs_host_view *main_view,
    const smvs_host_view *subs, int n_subs, const smvs_host_bundle *bundle,
    const float *sgm_depth, int sgm_w, int sgm_h, float *sgm_depth_roundtrip,
    const smvs_host_options *opts, unsigned flags, float *depth_out,
    float *normals_out, smvs_host_log *log);
/* The same with sgm_slant[slant_h][slant_w][slant_channels] (may be NULL: none)
 * stored as the "smvs-sgm-slant" embedding, as the SGM front end's refinement
 * sweeps would; smvs_host_optimize_flags forwards to this with NULL. */
int smvs_host_optimize_planes(const smvs_host_view *main_view,
    const smvs_host_view *subs, int n_subs, const smvs_host_bundle *bundle,
    const float *sgm_depth, int sgm_w, int sgm_h, float *sgm_depth_roundtrip,
    const float *sgm_slant, int slant_w, int slant_h, int slant_channels,
    const smvs_host_options *opts, unsigned flags, float *depth_out,
    float *normals_out, smvs_host_log *log);

/* The host's StereoView::initialize_linear (lib/stereo_view.cc:64-84) of a view
 * built from `bytes` (width x height x channels, interleaved): shading_out
 * (width x height floats) and grad_out (x 2), either may be NULL.
 * smvs_host_gamma_inv_srgb_lut: imgtools::gamma_inv_srgb_lut, the table
 * DepthOptimizer hands to smvs_ctx_prepare_shading.  Neither needs a device. */
int smvs_host_shading_planes(const uint8_t *bytes, int width, int height,
    int channels, int gamma, float *shading_out, float *grad_out);
int smvs_host_gamma_inv_srgb_lut(float *out256);

/* The embeddings the last smvs_host_optimize of this thread left in its main
 * view (write_depth_to_view / write_image_to_view: the result "smvs" / "smvsN",
 * and with Options::debug_lvl >= 2 -- SMVS_DEBUG_LVL -- the reference's
 * intermediate ones, lib/depth_optimizer.cc:44-45, 68-70, 119-156,
 * depth_optimizer.h:150-160).  names_out: the names, separated by newlines
 * (truncated to cap bytes); returns their number.  smvs_host_embedding copies
 * one (whc = width, height, channels; returns 0, -1 if there is none, or the
 * number of floats needed when cap_floats is too small). */
int smvs_host_embedding_names(char *names_out, int cap);
int smvs_host_embedding(const char *name, float *out, long long cap_floats, int *whc);

/* Loop recording (measurement, see RecordedLoop in depth_optimizer.h):
 * smvs_host_record_loops(1) drops what this thread recorded before (the clones
 * are destroyed) and starts recording, (0) stops; every smvs_host_optimize of
 * the thread in between leaves one entry per Newton batch.
 * smvs_host_recorded_loops copies up to `cap` entries -- context handle, loop
 * parameters (a smvs_gn_loop_params each), scale, iteration -- and returns how
 * many were recorded.  The contexts belong to the recorder until
 * smvs_host_release_recorded_loops: destroy != 0 destroys them, 0 hands them
 * to the caller (who ends each with smvs_ctx_destroy). */
int smvs_host_record_loops(int on);
int smvs_host_recorded_loops(void **ctxs, void *params, int *scales, int *iters,
    int cap);
int smvs_host_release_recorded_loops(int destroy);

/* reconstruct_sgm_depth_for_view (app/smvsrecon.cc:346-384): returns the
 * merged z-depth map at SGM resolution ((w+1)>>scale ...). */
int smvs_host_sgm_depth(const smvs_host_view *main_view,
    const smvs_host_view *subs, int n_subs, const smvs_host_bundle *bundle,
    int sgm_scale, float min_depth, float max_depth, int device,
    float *depth_out, int *out_w, int *out_h);
/* The same with SGMStereo::Options::adaptive_penalty2 (not in the reference's
 * Options: != 0 reproduces its build without SSE, lib/sgm_stereo.cc:310-346;
 * 0 is smvs_host_sgm_depth). */
int smvs_host_sgm_depth_mode(const smvs_host_view *main_view,
    const smvs_host_view *subs, int n_subs, const smvs_host_bundle *bundle,
    int sgm_scale, float min_depth, float max_depth, int device,
    int adaptive_penalty2, float *depth_out, int *out_w, int *out_h);
/* The same with SGMStereo::Options::num_steps, the number of inverse-depth
 * planes: 2 .. 128, or a multiple of 8 from 136 to 256 (include/smvs_hip.h,
 * "plane counts"); any other count is an argument error before anything runs.
 * smvs_host_sgm_depth and ..._mode forward to this with 128. */
int smvs_host_sgm_depth_steps(const smvs_host_view *main_view,
    const smvs_host_view *subs, int n_subs, const smvs_host_bundle *bundle,
    int sgm_scale, float min_depth, float max_depth, int device,
    int adaptive_penalty2, int num_steps, float *depth_out, int *out_w, int *out_h);
/* The same with SGMStereo::Options::subplane (not in the reference's Options:
 * != 0 refines every run's winning plane with the parabola through its
 * aggregated cost and its two neighbours', SMVS_SGM_WINNER_SUBPLANE of
 * include/smvs_hip.h; 0 is smvs_host_sgm_depth_steps, which forwards to this). */
int smvs_host_sgm_depth_subplane(const smvs_host_view *main_view,
    const smvs_host_view *subs, int n_subs, const smvs_host_bundle *bundle,
    int sgm_scale, float min_depth, float max_depth, int device,
    int adaptive_penalty2, int num_steps, int subplane, float *depth_out, int *out_w,
    int *out_h);
/* The same with SGMStereo::Options::num_neighbors / consensus / agree_ratio /
 * min_agree (not in the reference, which merges the first two neighbours): the
 * first min(n_subs, num_neighbors) neighbours, merged by consensus
 * (SMVS_SGM_MERGE_CONSENSUS of include/smvs_hip.h) when consensus != 0.
 * num_neighbors > 2 with consensus == 0 is an argument error, never a silent
 * truncation.  smvs_host_sgm_depth_subplane forwards to this with
 * (2, 0, 0.95f, 2), which takes the path and gives the bytes it always did. */
int smvs_host_sgm_depth_merge(const smvs_host_view *main_view,
    const smvs_host_view *subs, int n_subs, const smvs_host_bundle *bundle,
    int sgm_scale, float min_depth, float max_depth, int device,
    int adaptive_penalty2, int num_steps, int subplane, int num_neighbors,
    int consensus, float agree_ratio, int min_agree, float *depth_out, int *out_w,
    int *out_h);
/* The merge options as a default-constructed SGMStereo::Options and
 * ReconSettings hold them (no device involved): ints4 = { Options::
 * num_neighbors, consensus, min_agree, 0 }, then the same of ReconSettings::
 * sgm (an SGMStereo::Options) in ints4[4 .. 7]; ratios2 =
 * { Options::agree_ratio, ReconSettings::sgm.agree_ratio }. */
int smvs_host_sgm_merge_defaults(int *ints8, float *ratios2);
/* SGMStereo::Options::sweep / sweep_min_views / sweep_best_k /
 * sweep_support_cost / sweep_min_support (the multi-neighbour plane sweep of
 * include/smvs_hip.h; not in the reference); -1 in min_views, best_k and
 * min_support: the default at n neighbours (min(2, n), (n + 1) / 2, min(2, n)). */
typedef struct {
    int sweep;
    int min_views, best_k, support_cost, min_support;
} smvs_host_sgm_sweep;
/* smvs_host_sgm_depth_merge with the plane sweep selectable: with sweep->sweep
 * != 0 the map of the sweep over the first min(n_subs, num_neighbors)
 * neighbours (any count up to SMVS_MAX_SUBS).  sweep together with consensus is
 * an argument error.  sweep == NULL: off; smvs_host_sgm_depth_merge forwards to
 * this with NULL. */
int smvs_host_sgm_depth_sweep(const smvs_host_view *main_view,
    const smvs_host_view *subs, int n_subs, const smvs_host_bundle *bundle,
    int sgm_scale, float min_depth, float max_depth, int device,
    int adaptive_penalty2, int num_steps, int subplane, int num_neighbors,
    int consensus, float agree_ratio, int min_agree, const smvs_host_sgm_sweep *sweep,
    float *depth_out, int *out_w, int *out_h);
/* The sweep options as a default-constructed SGMStereo::Options (ints10[0 .. 4])
 * and ReconSettings (ints10[5 .. 9]) hold them, in the order of
 * smvs_host_sgm_sweep (no device involved). */
int smvs_host_sgm_sweep_defaults(int *ints10);
/* SGMStereo::Options::uniqueness / uniqueness_window / speckle_size /
 * speckle_ratio (the two filters of include/smvs_hip.h, "Two single-run
 * rejections"; not in the reference). */
typedef struct {
    int uniqueness, uniqueness_window, speckle_size;
    float speckle_ratio;
} smvs_host_sgm_filter;
/* smvs_host_sgm_depth_sweep with the filters, for any of the three front ends:
 * uniqueness outside 0 .. 99, a window outside 1 .. 256, a negative
 * speckle_size and a ratio outside [0, 1] are argument errors before anything
 * runs.  filter == NULL: off; smvs_host_sgm_depth_sweep forwards to this with
 * NULL. */
int smvs_host_sgm_depth_filtered(const smvs_host_view *main_view,
    const smvs_host_view *subs, int n_subs, const smvs_host_bundle *bundle,
    int sgm_scale, float min_depth, float max_depth, int device,
    int adaptive_penalty2, int num_steps, int subplane, int num_neighbors,
    int consensus, float agree_ratio, int min_agree, const smvs_host_sgm_sweep *sweep,
    const smvs_host_sgm_filter *filter, float *depth_out, int *out_w, int *out_h);
/* SGMStereo::Options::photo_radius / photo_best_k / photo_min_views /
 * photo_min_score / photo_witnesses (the multi-view photo-consistency test of
 * include/smvs_hip.h; not in the reference). */
typedef struct {
    int radius, best_k, min_views;
    float min_score;
    int witnesses;
} smvs_host_sgm_photo;
/* smvs_host_sgm_depth_filtered with the photo-consistency test, for any of the
 * three front ends: its witnesses are the first `witnesses` of subs (-1: all, 16
 * at the most; never fewer than the front end uses).  radius outside 0 .. 3,
 * best_k or min_views outside 0 .. 16, min_score outside [-1, 1] or NaN and
 * witnesses outside -1 .. 16 are argument errors before anything runs; the
 * device refuses a best_k or min_views above the witnesses there are.
 * confidence_out (may be NULL): the confidence map, written with the test on.
 * photo == NULL or radius 0: off; smvs_host_sgm_depth_filtered forwards to this
 * with NULL. */
int smvs_host_sgm_depth_photo(const smvs_host_view *main_view,
    const smvs_host_view *subs, int n_subs, const smvs_host_bundle *bundle,
    int sgm_scale, float min_depth, float max_depth, int device,
    int adaptive_penalty2, int num_steps, int subplane, int num_neighbors,
    int consensus, float agree_ratio, int min_agree, const smvs_host_sgm_sweep *sweep,
    const smvs_host_sgm_filter *filter, const smvs_host_sgm_photo *photo, float *depth_out,
    float *confidence_out, int *out_w, int *out_h);
/* SGMStereo::Options::refine_sweeps / refine_samples / refine_depth_step /
 * refine_slant_step / refine_seed / refine_fill (the multi-view plane refinement
 * sweeps of include/smvs_hip.h; not in the reference). */
typedef struct {
    int sweeps, samples;
    float depth_step, slant_step;
    uint32_t seed;
    int fill;
} smvs_host_sgm_refine;
/* smvs_host_sgm_depth_photo with the refinement sweeps in the photo test's place,
 * for any of the three front ends.  sweeps or samples outside 0 .. 8, a step
 * outside [0, 1] or NaN and fill other than 0 or 1 are argument errors before
 * anything runs; the device refuses sweeps > 0 with the photo test off.
 * slant_out (may be NULL): the slants [h][w][2], written with the sweeps on.
 * refine == NULL or sweeps 0: off; smvs_host_sgm_depth_photo forwards to this
 * with NULL. */
int smvs_host_sgm_depth_refine(const smvs_host_view *main_view,
    const smvs_host_view *subs, int n_subs, const smvs_host_bundle *bundle,
    int sgm_scale, float min_depth, float max_depth, int device,
    int adaptive_penalty2, int num_steps, int subplane, int num_neighbors,
    int consensus, float agree_ratio, int min_agree, const smvs_host_sgm_sweep *sweep,
    const smvs_host_sgm_filter *filter, const smvs_host_sgm_photo *photo,
    const smvs_host_sgm_refine *refine, float *depth_out, float *confidence_out,
    float *slant_out, int *out_w, int *out_h);
/* The refine options as a default-constructed SGMStereo::Options (ints8[0 .. 3],
 * steps4[0 .. 1]) and ReconSettings (ints8[4 .. 7], steps4[2 .. 3]) hold them:
 * sweeps, samples, seed, fill; depth_step, slant_step (no device involved). */
int smvs_host_sgm_refine_defaults(int *ints8, float *steps4);
/* The photo options as a default-constructed SGMStereo::Options (ints8[0 .. 3],
 * scores2[0]) and ReconSettings (ints8[4 .. 7], scores2[1]) hold them: radius,
 * best_k, min_views, witnesses; min_score (no device involved). */
int smvs_host_sgm_photo_defaults(int *ints8, float *scores2);
/* The filter options as a default-constructed SGMStereo::Options (ints6[0 .. 2],
 * ratios2[0]) and ReconSettings (ints6[3 .. 5], ratios2[1]) hold them, in the
 * order of smvs_host_sgm_filter (no device involved). */
int smvs_host_sgm_filter_defaults(int *ints6, float *ratios2);
/* The switches of the SGM front end that the reference does not have, as a
 * default-constructed SGMStereo::Options and ReconSettings hold them (no
 * device involved): out4 = { Options::adaptive_penalty2, Options::subplane,
 * ReconSettings::sgm.adaptive_penalty2, ReconSettings::sgm.subplane }. */
int smvs_host_sgm_default_switches(int *out4);

/* smvs::Surface on its own (lib/surface.cc): Surface::create (from the bundle
 * when init_depth is NULL, else from the W x H depth map) followed by a
 * script of operations -- 1 expand, 2 subdivide_patches,
 * 3 fill_patches_from_depth, 4 remove_isolated_patches, 5 delete every
 * delete_every-th valid patch + remove_nodes_without_patch.  No device
 * involved.  info = { scale, npx, npy, start_x, start_y }; the arrays are
 * caller-sized (for the finest scale the script reaches). */
int smvs_host_surface_script(const smvs_host_view *main_view,
    const smvs_host_bundle *bundle, const float *init_depth, int init_scale,
    const int *ops, int n_ops, int delete_every, int *info, double *nodes_out,
    uint8_t *node_valid_out, uint8_t *patch_valid_out);
/* The same script on the surface of a device context (include/smvs_hip.h,
 * "grid surgery"); info[5] = valid patches as the last operation reported. */
int smvs_host_surface_script_device(const smvs_host_view *main_view,
    const smvs_host_bundle *bundle, const float *init_depth, int init_scale,
    const int *ops, int n_ops, int delete_every, int device, int *info6,
    double *nodes_out, uint8_t *node_valid_out, uint8_t *patch_valid_out);
/* The two with a slant plane: init_depth (W x H) and init_slant (W x H x 2, the
 * plane P of include/smvs_hip.h, "Node slopes from the SGM plane hypotheses")
 * are both required; Surface::create(..., init, slant) on the host,
 * smvs_surface_create_planes on the device. */
int smvs_host_surface_script_planes(const smvs_host_view *main_view,
    const float *init_depth, const float *init_slant, int init_scale,
    const int *ops, int n_ops, int delete_every, int *info, double *nodes_out,
    uint8_t *node_valid_out, uint8_t *patch_valid_out);
int smvs_host_surface_script_planes_device(const smvs_host_view *main_view,
    const float *init_depth, const float *init_slant, int init_scale,
    const int *ops, int n_ops, int delete_every, int device, int *info6,
    double *nodes_out, uint8_t *node_valid_out, uint8_t *patch_valid_out);
/* Surface::slant_plane, the tap rule of smvs_ctx_sgm_init_slants on the host (no
 * device involved): lowres[dm_h][dm_w], slants[dm_h][dm_w][2] ->
 * out[height][width][2]. */
int smvs_host_slant_plane(const float *lowres, const float *slants, int dm_w, int dm_h,
    int width, int height, float *out);

/* The per-view tasks of smvsrecon (app/smvsrecon.cc:658-733) for n_jobs
 * reference views on a smvs_amd::ViewQueue: per job StereoView::create for the
 * main view and its neighbours, optionally reconstruct_sgm_depth_for_view
 * (sgm_scale >= 0; a negative value skips the SGM front end and initialises
 * from the bundle), DepthOptimizer(...).optimize(), depth + normal maps.
 * Job i uses mains[i] and subs[i * n_subs .. (i + 1) * n_subs).  Worker w runs
 * on device first_device + w % num_devices with views_in_flight workers per
 * device.  Outputs (each may be NULL): depth_out / normals_out of job
 * `keep_job` only (W * H and W * H * 3 floats of that job's main view),
 * job_seconds[n_jobs] = wall time of each task, *total_seconds = wall time
 * from the first task queued to the last finished, logs[n_jobs]. */
int smvs_host_optimize_views(const smvs_host_view *mains,
    const smvs_host_view *subs, int n_jobs, int n_subs,
    const smvs_host_bundle *bundle, const smvs_host_options *opts, int sgm_scale,
    int first_device, int num_devices, int views_in_flight, int keep_job,
    float *depth_out, float *normals_out, double *job_seconds,
    double *total_seconds, smvs_host_log *logs);

/* The reference's own Newton-step calls through the compatibility classes
 * (lib/depth_optimizer.cc:225-262): Surface::create(bundle, main, init_scale),
 * StereoView::set_scale(scale of the surface) on every view (host planes),
 * GaussNewtonStep(opts, main, subs, Mi, ti).construct(surface, subsurfaces =
 * every neighbour for every patch, active = every node, lighting = NULL, &H,
 * &g, &P), then ConjugateGradient({200, 0.01 |g|, 1e-3}).solve(H, -g, &x, &P).
 * Outputs (caller-sized, each may be NULL): the planes the step used --
 * main_grad[W*H*2], sub_grad[n_subs][W*H*2], sub_hess[n_subs][W*H*3] -- the
 * reprojections Mi[n_subs*9], ti[n_subs*3], flen2 = { flen, inverse flen }, and
 * g[4N], x[4N], H9[N*9*16], P[N*16], cg = { iterations, info }. */
int smvs_host_gn_solve_step(const smvs_host_view *main_view,
    const smvs_host_view *subs, int n_subs, const smvs_host_bundle *bundle,
    int init_scale, double regularization, int device, float *main_grad,
    float *sub_grad, float *sub_hess, double *Mi, double *ti, float *flen2,
    double *g, double *x, double *H9, double *P, int *cg);

/* smvsrecon's scene-level run (app/smvsrecon.cc:400-745) on an MVE scene
 * directory whose input embedding exists as <image_embedding>.mvei: view list,
 * ViewSelection, one ViewQueue task per reference view, result embeddings
 * written into the view directories.  view_ids may be NULL (every view).
 * reconstructed_out[max_reconstructed] receives the ids of the reconstructed
 * views (may be NULL with max_reconstructed = 0); *n_reconstructed is their
 * number -- when it exceeds max_reconstructed only the first
 * max_reconstructed ids were stored (the scene has been reconstructed; the
 * caller can size the buffer from smvs_host_scene_info). */
typedef struct {
    const char *image_embedding;    /* "undistorted" */
    float regularization;           /* alpha, 1.0 */
    int output_scale;               /* -o */
    int use_shading, use_sgm, force_recon, force_sgm, full_optimization;
    float sgm_min, sgm_max;
    int sgm_scale;
    int num_neighbors, min_neighbors;
    int first_device, num_devices, views_in_flight;
    int input_scale;                /* -s; < 0: automatic (app/smvsrecon.cc:477-500) */
    int max_pixels;                 /* --max-pixels, 1700000 */
} smvs_host_recon_settings;
int smvs_host_reconstruct_scene(const char *scene_dir,
    const smvs_host_recon_settings *settings, const int *view_ids, int n_view_ids,
    int *reconstructed_out, int max_reconstructed, int *n_reconstructed,
    int *n_skipped, double *seconds, int *input_scale_used);
/* The same with ReconSettings::sgm.adaptive_penalty2 (the settings struct keeps
 * its layout for existing callers, so the switch is an argument: != 0 runs the
 * SGM front end of every view as the reference's build without SSE does,
 * lib/sgm_stereo.cc:310-346; 0 is smvs_host_reconstruct_scene). */
int smvs_host_reconstruct_scene_mode(const char *scene_dir,
    const smvs_host_recon_settings *settings, int sgm_adaptive_penalty2,
    const int *view_ids, int n_view_ids, int *reconstructed_out, int max_reconstructed,
    int *n_reconstructed, int *n_skipped, double *seconds, int *input_scale_used);

/* The same with a word of switches the settings struct does not hold (it keeps
 * its layout for existing callers).  Bit 0: ReconSettings::sgm.adaptive_penalty2
 * (smvs_host_reconstruct_scene_mode's argument); bit 1: ReconSettings::
 * device_input_scaling -- the input scaling of app/smvsrecon.cc:621-650 runs on
 * the device (smvs_rescale_half_gaussian), one ViewQueue task per view; the
 * undist-L<s> images are the host path's, bit for bit; bit 3: ReconSettings::
 * device_shading_prep -- with use_shading, every view's shading planes
 * (lib/stereo_view.cc:64-84) are made on the device (smvs_ctx_prepare_shading),
 * the embeddings are the host path's, bit for bit; bit 4: ReconSettings::
 * gamma_correction (app/smvsrecon.cc:52, 669), which the struct has no field
 * for.  An unknown bit is an argument error.  smvs_host_reconstruct_scene and ..._mode forward to this. */
#define SMVS_HOST_SCENE_ADAPTIVE_PENALTY2 1
#define SMVS_HOST_SCENE_DEVICE_INPUT_SCALING 2
/* (value 4 is not assigned: it stays the argument error callers have met so far) */
#define SMVS_HOST_SCENE_DEVICE_SHADING_PREP 8   /* ReconSettings::device_shading_prep */
#define SMVS_HOST_SCENE_GAMMA_SRGB 16           /* ReconSettings::gamma_correction (--gamma-srgb) */
/* ReconSettings::init_slants: the initial surfaces' node slopes from the views'
 * smvs-sgm-slant embeddings.  Known to smvs_host_reconstruct_scene_planes only
 * (to the entries before it, it stays the unknown bit it was); an argument
 * error before the scene is read unless the refinement sweeps are on. */
#define SMVS_HOST_SCENE_INIT_SLANTS 32
int smvs_host_reconstruct_scene_flags(const char *scene_dir,
    const smvs_host_recon_settings *settings, unsigned flags, const int *view_ids,
    int n_view_ids, int *reconstructed_out, int max_reconstructed, int *n_reconstructed,
    int *n_skipped, double *seconds, int *input_scale_used);
/* The same with ReconSettings::sgm.num_steps, the inverse-depth planes of every
 * view's SGM front end (the settings struct keeps its layout): 2 .. 128, or a
 * multiple of 8 from 136 to 256; any other count is an argument error before
 * the scene is read.  smvs_host_reconstruct_scene_flags forwards to this with
 * 128. */
int smvs_host_reconstruct_scene_steps(const char *scene_dir,
    const smvs_host_recon_settings *settings, unsigned flags, int sgm_num_steps,
    const int *view_ids, int n_view_ids, int *reconstructed_out, int max_reconstructed,
    int *n_reconstructed, int *n_skipped, double *seconds, int *input_scale_used);
/* The same with ReconSettings::sgm.subplane (an argument: the settings struct
 * keeps its layout and the flags word its known bits): != 0 runs every view's
 * SGM front end with SGMStereo::Options::subplane.  An smvs-sgm embedding of
 * the right size is reused as before (app/smvsrecon.cc:702-708), so a scene
 * that already has one needs force_sgm as well.
 * smvs_host_reconstruct_scene_steps forwards to this with 0. */
int smvs_host_reconstruct_scene_subplane(const char *scene_dir,
    const smvs_host_recon_settings *settings, unsigned flags, int sgm_num_steps,
    int sgm_subplane, const int *view_ids, int n_view_ids, int *reconstructed_out,
    int max_reconstructed, int *n_reconstructed, int *n_skipped, double *seconds,
    int *input_scale_used);
/* The same with ReconSettings::sgm.num_neighbors / consensus / agree_ratio /
 * min_agree (arguments: the settings struct keeps its layout): every view's
 * smvs-sgm map from its first sgm_neighbors neighbours (capped by the
 * neighbours the view has), merged by consensus when sgm_consensus != 0;
 * sgm_neighbors > 2 without it is an argument error.  The reuse rule is that of
 * sgm_subplane: a scene that already has smvs-sgm embeddings needs force_sgm.
 * smvs_host_reconstruct_scene_subplane forwards to this with (2, 0, 0.95f, 2). */
int smvs_host_reconstruct_scene_merge(const char *scene_dir,
    const smvs_host_recon_settings *settings, unsigned flags, int sgm_num_steps,
    int sgm_subplane, int sgm_neighbors, int sgm_consensus, float sgm_agree_ratio,
    int sgm_min_agree, const int *view_ids, int n_view_ids, int *reconstructed_out,
    int max_reconstructed, int *n_reconstructed, int *n_skipped, double *seconds,
    int *input_scale_used);
/* The same with ReconSettings::sgm.sweep and its four values: every view's
 * smvs-sgm map by the plane sweep over its first sgm_neighbors neighbours.
 * sweep together with sgm_consensus is an argument error; sweep == NULL: off
 * (smvs_host_reconstruct_scene_merge forwards to this with NULL).  The reuse
 * rule is that of sgm_subplane (force_sgm). */
int smvs_host_reconstruct_scene_sweep(const char *scene_dir,
    const smvs_host_recon_settings *settings, unsigned flags, int sgm_num_steps,
    int sgm_subplane, int sgm_neighbors, int sgm_consensus, float sgm_agree_ratio,
    int sgm_min_agree, const smvs_host_sgm_sweep *sweep, const int *view_ids,
    int n_view_ids, int *reconstructed_out, int max_reconstructed, int *n_reconstructed,
    int *n_skipped, double *seconds, int *input_scale_used);

/* The same with ReconSettings::sgm.uniqueness / uniqueness_window /
 * speckle_size / speckle_ratio: the two filters in every view's SGM
 * front end (arguments: the settings struct keeps its layout).  A value outside
 * the accepted set is an argument error before the scene is read; filter ==
 * NULL: off (smvs_host_reconstruct_scene_sweep forwards to this with NULL).  The
 * reuse rule is that of sgm_subplane (force_sgm). */
int smvs_host_reconstruct_scene_filtered(const char *scene_dir,
    const smvs_host_recon_settings *settings, unsigned flags, int sgm_num_steps,
    int sgm_subplane, int sgm_neighbors, int sgm_consensus, float sgm_agree_ratio,
    int sgm_min_agree, const smvs_host_sgm_sweep *sweep, const smvs_host_sgm_filter *filter,
    const int *view_ids, int n_view_ids, int *reconstructed_out, int max_reconstructed,
    int *n_reconstructed, int *n_skipped, double *seconds, int *input_scale_used);

/* The same with ReconSettings::sgm.photo_radius / photo_best_k /
 * photo_min_views / photo_min_score / photo_witnesses: the
 * photo-consistency test behind every view's SGM front end, the confidence saved
 * as smvs-sgm-confidence.  A value outside the accepted set is an argument error
 * before the scene is read; photo == NULL: off
 * (smvs_host_reconstruct_scene_filtered forwards to this with NULL).  The reuse
 * rule is that of sgm_subplane (force_sgm). */
int smvs_host_reconstruct_scene_photo(const char *scene_dir,
    const smvs_host_recon_settings *settings, unsigned flags, int sgm_num_steps,
    int sgm_subplane, int sgm_neighbors, int sgm_consensus, float sgm_agree_ratio,
    int sgm_min_agree, const smvs_host_sgm_sweep *sweep, const smvs_host_sgm_filter *filter,
    const smvs_host_sgm_photo *photo, const int *view_ids, int n_view_ids,
    int *reconstructed_out, int max_reconstructed, int *n_reconstructed, int *n_skipped,
    double *seconds, int *input_scale_used);

/* The same with ReconSettings::sgm.refine_sweeps / refine_samples /
 * refine_depth_step / refine_slant_step / refine_seed /
 * refine_fill: the plane refinement sweeps in the photo test's place, the
 * slants saved as smvs-sgm-slant (two channels) next to smvs-sgm-confidence.  A
 * value outside the accepted set is an argument error before the scene is read;
 * refine == NULL: off (smvs_host_reconstruct_scene_photo forwards to this with
 * NULL).  The reuse rule is that of sgm_subplane (force_sgm). */
int smvs_host_reconstruct_scene_refine(const char *scene_dir,
    const smvs_host_recon_settings *settings, unsigned flags, int sgm_num_steps,
    int sgm_subplane, int sgm_neighbors, int sgm_consensus, float sgm_agree_ratio,
    int sgm_min_agree, const smvs_host_sgm_sweep *sweep, const smvs_host_sgm_filter *filter,
    const smvs_host_sgm_photo *photo, const smvs_host_sgm_refine *refine, const int *view_ids,
    int n_view_ids, int *reconstructed_out, int max_reconstructed, int *n_reconstructed,
    int *n_skipped, double *seconds, int *input_scale_used);

/* The same with SMVS_HOST_SCENE_INIT_SLANTS among the flags
 * (ReconSettings::init_slants); smvs_host_reconstruct_scene_refine forwards
 * here with its own set of bits. */
int smvs_host_reconstruct_scene_planes(const char *scene_dir,
    const smvs_host_recon_settings *settings, unsigned flags, int sgm_num_steps,
    int sgm_subplane, int sgm_neighbors, int sgm_consensus, float sgm_agree_ratio,
    int sgm_min_agree, const smvs_host_sgm_sweep *sweep, const smvs_host_sgm_filter *filter,
    const smvs_host_sgm_photo *photo, const smvs_host_sgm_refine *refine, const int *view_ids,
    int n_view_ids, int *reconstructed_out, int max_reconstructed, int *n_reconstructed,
    int *n_skipped, double *seconds, int *input_scale_used);

/* smvsrecon's generate_mesh (app/smvsrecon.cc:278-343, MeshGenerator::
 * generate_mesh, lib/mesh_generator.cc:160-299) on a reconstructed scene: the
 * point cloud of the views' <dm_name> / <dm_name>N / <input> embeddings (cut
 * on the device, smvs_points_generate), smvs-cut.mvei per view when cutting,
 * the AABB clip, <scene>/smvs-{B,S}<input_scale>.ply.  create_triangle_mesh
 * (--mesh: smvs_host_generate_mesh) and simplify (--simplify:
 * smvs_host_generate_simplified) are refused.  view_ids may be NULL
 * (every view).  ply_path (may be NULL) receives the file name. */
typedef struct {
    const char *image_embedding;    /* "undistorted" */
    int input_scale;                /* the scale the scene was reconstructed at */
    int use_shading;                /* names smvs-S / smvs-B */
    int cut_surface;                /* 0: --no-cut */
    int create_triangle_mesh;       /* --mesh: refused */
    int simplify;                   /* --simplify: refused (smvs_host_generate_simplified) */
    int use_aabb;
    float aabb_min[3], aabb_max[3];
    int device;
} smvs_host_point_cloud_settings;
int smvs_host_generate_point_cloud(const char *scene_dir,
    const smvs_host_point_cloud_settings *settings, const int *view_ids,
    int n_view_ids, char *ply_path, int ply_path_capacity, int64_t *n_points);
/* save_ply_points: the PLY writer of the point cloud from SoA buffers
 * (xyz, normals n*3 floats; rgb n*3 bytes; confidence, value n floats). */
int smvs_host_save_ply_points(const char *path, const float *xyz, const float *normals,
    const uint8_t *rgb, const float *confidence, const float *value, int64_t n);
/* smvsrecon --mesh (app/smvsrecon.cc:278-343 with create_triangle_mesh):
 * the triangle mesh of the same views (smvs_mesh_generate: merged, AABB
 * clip with delete_vertices_fix_faces, recalc_normals), smvs-cut.mvei per
 * view when cutting, <scene>/smvs-m-{B,S}<input_scale>.ply.  The settings are
 * the point cloud's (create_triangle_mesh is implied and ignored); simplify
 * (--simplify) is refused: smvs_host_generate_simplified. */
int smvs_host_generate_mesh(const char *scene_dir,
    const smvs_host_point_cloud_settings *settings, const int *view_ids,
    int n_view_ids, char *ply_path, int ply_path_capacity, int64_t *n_vertices,
    int64_t *n_faces);
/* smvsrecon --simplify (and --mesh --simplify with create_triangle_mesh):
 * approximate_triangulation per view on the device (smvs_simplified_generate,
 * DESIGN.md section 9.7), smvs-cut.mvei per view when cutting, the reference's
 * file names: <scene>/smvs-{B,S}<input_scale>.ply, with the mesh
 * smvs-m-{B,S}<input_scale>.ply.  The settings are the point cloud's; simplify
 * is implied and ignored.  *n_faces is 0 for the point cloud. */
int smvs_host_generate_simplified(const char *scene_dir,
    const smvs_host_point_cloud_settings *settings, const int *view_ids,
    int n_view_ids, char *ply_path, int ply_path_capacity, int64_t *n_vertices,
    int64_t *n_faces);
/* Not in the reference: the views' depth maps fused into ONE surface mesh
 * (smvs_tsdf_fuse), <scene>/smvs-fused-{B,S}
 * <input_scale>.ply through save_ply_mesh; no smvs-cut is written.  The
 * settings are the point cloud's (create_triangle_mesh and simplify are
 * ignored); with use_aabb the box is [aabb_min, aabb_max], else
 * smvs_tsdf_bounds padded by the truncation distance.  voxel_size <= 0: the
 * box's longest side / resolution; trunc <= 0: 3 voxels; min_weight <= 0: 1.
 * dims[a] = max(2, (int)ceilf((hi[a] - lo[a]) / voxel_size)). */
typedef struct {
    float voxel_size;
    int resolution;
    float trunc;
    int min_weight;
} smvs_host_fused_settings;
int smvs_host_generate_fused(const char *scene_dir,
    const smvs_host_point_cloud_settings *settings, const smvs_host_fused_settings *fused,
    const int *view_ids, int n_view_ids, char *ply_path, int ply_path_capacity,
    int64_t *n_vertices, int64_t *n_faces);
/* smvs_host_generate_fused on the brick-sparse volume (smvs_tsdf_fuse_sparse,
 * DESIGN.md section 9.9): the same file name, the same mesh with vertices and
 * faces in the brick order.  resolution (and every dim) may go up to 4096;
 * max_bricks <= 0: 1 << 20.  More bricks needed than max_bricks is an error
 * whose text names the count. */
typedef struct {
    float voxel_size;
    int resolution;
    float trunc;
    int min_weight;
    int64_t max_bricks;
} smvs_host_fused_sparse_settings;
int smvs_host_generate_fused_sparse(const char *scene_dir,
    const smvs_host_point_cloud_settings *settings,
    const smvs_host_fused_sparse_settings *fused, const int *view_ids, int n_view_ids,
    char *ply_path, int ply_path_capacity, int64_t *n_vertices, int64_t *n_faces);
/* smvs_host_generate_fused_sparse through smvs_tsdf_fuse_sparse_opts (DESIGN.md
 * section 9.10): with cull != 0 the brick cull against the views' depth min/max
 * pyramids runs in front of the seed pass; the file is the same byte for byte. */
typedef struct {
    float voxel_size;
    int resolution;
    float trunc;
    int min_weight;
    int64_t max_bricks;
    int cull;
} smvs_host_fused_sparse_cull_settings;
int smvs_host_generate_fused_sparse_cull(const char *scene_dir,
    const smvs_host_point_cloud_settings *settings,
    const smvs_host_fused_sparse_cull_settings *fused, const int *view_ids, int n_view_ids,
    char *ply_path, int ply_path_capacity, int64_t *n_vertices, int64_t *n_faces);
/* The fused mesh of one of the three entries above -- dense (sparse == 0;
 * max_bricks and cull must then be 0), sparse, or sparse with cull != 0 --
 * cleaned by smvs_mesh_clean_handle (threshold,
 * percentile, component_size, keep_unreferenced are smvs_mesh_clean_options')
 * and written through save_ply_mesh as <scene>/smvs-clean-{B,S}<input_scale>
 * .ply; the fused file is not written.  The record's first six members are the
 * cull entry's.  n_vertices and n_faces are the cleaned mesh's; stats (may be
 * NULL) what the clean counted. */
typedef struct {
    float voxel_size;
    int resolution;
    float trunc;
    int min_weight;
    int64_t max_bricks;
    int cull;
    int sparse;
    float threshold;
    float percentile;
    int component_size;
    int keep_unreferenced;
} smvs_host_fused_clean_settings;
int smvs_host_generate_fused_clean(const char *scene_dir,
    const smvs_host_point_cloud_settings *settings,
    const smvs_host_fused_clean_settings *fused, const int *view_ids, int n_view_ids,
    char *ply_path, int ply_path_capacity, int64_t *n_vertices, int64_t *n_faces,
    smvs_mesh_clean_stats *stats);
/* The dense fused mesh with only batch_views consecutive scene views loaded at
 * a time: the bounds are folded batch by batch, the
 * batches are integrated into a persistent volume (smvs_tsdf_volume) and the
 * surface is extracted once.  Without the cut (cut_surface == 0) the file is
 * smvs_host_generate_fused's byte for byte; the cut, when on, acts within a
 * batch.  The record's first eleven members are the clean entry's; clean != 0
 * cleans the mesh as that entry does (file name, counts, stats), clean == 0
 * writes the fused file and leaves stats alone.  batch_views == 0 is the
 * unbatched entry (dense or sparse as the record says); batch_views > 0 with
 * sparse != 0 is refused, and so is batch_views < 0. */
typedef struct {
    float voxel_size;
    int resolution;
    float trunc;
    int min_weight;
    int64_t max_bricks;
    int cull;
    int sparse;
    float threshold;
    float percentile;
    int component_size;
    int keep_unreferenced;
    int clean;
    int batch_views;
} smvs_host_fused_batched_settings;
int smvs_host_generate_fused_batched(const char *scene_dir,
    const smvs_host_point_cloud_settings *settings,
    const smvs_host_fused_batched_settings *fused, const int *view_ids, int n_view_ids,
    char *ply_path, int ply_path_capacity, int64_t *n_vertices, int64_t *n_faces,
    smvs_mesh_clean_stats *stats);
/* The brick-sparse fused mesh with only sparse_batch_views consecutive scene
 * views loaded at a time: three passes over the scene
 * -- the bounds folded batch by batch (skipped with use_aabb), every batch
 * marked (with cull != 0 the brick cull in front), every batch integrated
 * without growth -- into a persistent brick-sparse volume
 * (smvs_tsdf_sparse_volume), and the surface extracted once.  Without the cut
 * (cut_surface == 0) the file is smvs_host_generate_fused_sparse's byte for
 * byte; the cut, when on, acts within a batch.  The record's first thirteen
 * members are the batched entry's, and mean what they mean there (batch_views
 * > 0 with sparse != 0 stays refused); sparse_batch_views == 0 is that entry,
 * sparse_batch_views > 0 needs sparse != 0, and < 0 is refused. */
typedef struct {
    float voxel_size;
    int resolution;
    float trunc;
    int min_weight;
    int64_t max_bricks;
    int cull;
    int sparse;
    float threshold;
    float percentile;
    int component_size;
    int keep_unreferenced;
    int clean;
    int batch_views;
    int sparse_batch_views;
} smvs_host_fused_sparse_batched_settings;
int smvs_host_generate_fused_sparse_batched(const char *scene_dir,
    const smvs_host_point_cloud_settings *settings,
    const smvs_host_fused_sparse_batched_settings *fused, const int *view_ids, int n_view_ids,
    char *ply_path, int ply_path_capacity, int64_t *n_vertices, int64_t *n_faces,
    smvs_mesh_clean_stats *stats);
/* save_ply_mesh: the PLY writer of the triangle mesh from SoA
 * buffers (xyz, normals n*3 floats; rgb n*3 bytes; confidence n floats;
 * faces m*3 vertex ids < n). */
int smvs_host_save_ply_mesh(const char *path, const float *xyz, const float *normals,
    const uint8_t *rgb, const float *confidence, int64_t n, const uint32_t *faces,
    int64_t m);

/* Byte-image containers of a view directory (csrc/host/png_io.cc,
 * scene_io.cc): load `path` (.png or .mvei, u8) -> width, height, channels and,
 * if pixels != NULL with room for capacity bytes, the interleaved data;
 * save a u8 image as PNG; mve::image::rescale_half_size_gaussian<uint8_t>
 * (out sized ((w + 1) / 2) * ((h + 1) / 2) * c). */
int smvs_host_load_byte_image(const char *path, int *whc, uint8_t *pixels,
    size_t capacity);
int smvs_host_save_png(const char *path, const uint8_t *pixels, int width, int height,
    int channels);
int smvs_host_rescale_half_size_gaussian(const uint8_t *pixels, int width, int height,
    int channels, uint8_t *out);
/* `halvings` of them chained on device `device` (smvs_rescale_half_gaussian,
 * app/smvsrecon.cc:634-647), bit-identical with the host function applied
 * `halvings` times; out has room for out_capacity bytes, *out_width /
 * *out_height receive the last level's size. */
int smvs_host_rescale_half_size_gaussian_device(const uint8_t *pixels, int width,
    int height, int channels, int halvings, int device, uint8_t *out,
    size_t out_capacity, int *out_width, int *out_height);

/* COLMAP models as MVE scenes (csrc/host/colmap_io.h; [COLMAP-unverified] C1-C9
 * of tests/golden/COLMAP.md; no counterpart in the reference).
 *
 * smvs_host_undistort_u8: the undistortion resampling of include/smvs_hip.h;
 * device = -1: the host form (csrc/host/undistort_math.h, the kernel's own
 * arithmetic), device = k: smvs_undistort_u8 on device k; the same bytes and
 * the same blank count.  What smvs_undistort_u8 refuses is refused here, with
 * out untouched.
 *
 * smvs_host_read_colmap_model: cameras / images / points3D of model_dir (.bin
 * if all three are there, else .txt), checked, as three sections in COLMAP's
 * binary layout (C6-C8) one behind the other.  section_bytes3 receives their
 * sizes; buffer may be NULL to ask for the sizes first.  *binary: which files
 * were read.
 *
 * smvs_host_import_colmap: import_colmap.  container: 0 = png, 1 = mvei;
 * device -1: the host form; threads 1..16.  The per-view arrays (any may be
 * NULL) have room for max_views entries and receive the views written, in view
 * order: the view id, COLMAP's IMAGE_ID, width / height / channels, flen and
 * the number of blank pixels. */
typedef struct {
    int device;
    float zoom;
    int out_width, out_height;
    int container;
    int threads;
    int overwrite;
} smvs_host_import_settings;
typedef struct {
    int num_views, views_written;
    int64_t points_kept, points_dropped, track_elements_kept, track_elements_dropped;
    double seconds, decode_seconds, undistort_seconds, encode_seconds;
} smvs_host_import_report;
int smvs_host_undistort_u8(const uint8_t *pixels, int width, int height, int channels,
    const smvs_lens *lens, float out_focal, int out_width, int out_height, int device,
    uint8_t *out, int64_t *blank_pixels);
int smvs_host_read_colmap_model(const char *model_dir, uint8_t *buffer, size_t capacity,
    uint64_t *section_bytes3, int *binary);
int smvs_host_import_colmap(const char *model_dir, const char *image_dir,
    const char *scene_dir, const smvs_host_import_settings *settings, const int *view_ids,
    int n_view_ids, smvs_host_import_report *report, int max_views, int *view_id,
    uint32_t *image_id, int *whc3, float *flen, int64_t *blank_pixels);

/* MVE scene I/O without a device: parses the scene (views/<x>.mve/meta.ini,
 * synth_0.out) -> number of list entries, and per entry (caller-sized arrays of
 * at least max_views): present, flen, rot[9], trans[3], and the size of the
 * image embedding (0 x 0 when missing); *n_features of the bundle (-1: none).
 * mvei_roundtrip: loads in_path (u8 or float .mvei) and saves it to out_path. */
int smvs_host_scene_info(const char *scene_dir, const char *image_embedding,
    int max_views, int *n_views, int *present, float *flen, float *rot9,
    float *trans3, int *width, int *height, int *n_features);
int smvs_host_mvei_roundtrip(const char *in_path, const char *out_path);

/* smvs_amd::ViewQueue on its own (no device involved): n_tasks tasks that
 * record the slot they ran on; task `throwing_task` (or -1) throws.
 * device_hist[num_devices] and worker_hist[num_devices * views_in_flight]
 * receive the number of tasks per device / worker.  Returns 0 when every task
 * ran exactly once, the throwing task's exception arrived through its future
 * and no other future carried one. */
int smvs_host_view_queue_selftest(int n_tasks, int num_devices,
    int views_in_flight, int throwing_task, int *device_hist, int *worker_hist);

/* DepthOptimizer(main, subs, Surface::Ptr, opts) followed by get_depth() /
 * get_normals() WITHOUT optimize() (lib/depth_optimizer.h:53-61): the maps of
 * the surface Surface::create builds (from the bundle, or from init_depth). */
int smvs_host_surface_maps(const smvs_host_view *main_view,
    const smvs_host_view *subs, int n_subs, const smvs_host_bundle *bundle,
    const float *init_depth, int init_scale, int device, float *depth_out,
    float *normals_out);
/* The same for Surface::create(..., init_depth, init_slant): both required.
 * smvs_host_surface_maps_host: Surface::get_depth_map / get_normal_map of the
 * host mirror on their own, no device involved (init_slant may be NULL, either
 * output may be NULL). */
int smvs_host_surface_maps_host(const smvs_host_view *main_view, const float *init_depth,
    const float *init_slant, int init_scale, float *depth_out, float *normals_out);
int smvs_host_surface_maps_planes(const smvs_host_view *main_view,
    const smvs_host_view *subs, int n_subs, const smvs_host_bundle *bundle,
    const float *init_depth, const float *init_slant, int init_scale, int device,
    float *depth_out, float *normals_out);

/* Host-only pieces of the SGM front end, for CPU tests (no device involved):
 *   smvs_host_depth_range: SGMStereo::fill_depth_range_for_view
 *     (lib/sgm_stereo.cc:669-720) -> range[2];
 *   smvs_host_reprojection: CameraInfo::fill_reprojection from `source` to
 *     `destination` at their image sizes -> M[9], t[3] (lib/sgm_stereo.cc:56-62);
 *   smvs_host_sgm_image: StereoView::get_byte_image (desaturate<uint8_t>,
 *     lib/stereo_view.cc:86-95) followed by `halvings` rescale_half_size
 *     (lib/sgm_stereo.cc:31-39) -> out (caller-sized), *out_w, *out_h. */
int smvs_host_depth_range(const smvs_host_view *view,
    const smvs_host_bundle *bundle, float *range2);
int smvs_host_reprojection(const smvs_host_view *source,
    const smvs_host_view *destination, float *M9, float *t3);
int smvs_host_sgm_image(const smvs_host_view *view, int halvings, uint8_t *out,
    int *out_w, int *out_h);

/* smvs::ViewSelection(opts, views, bundle).get_neighbors_for_view(view)
 * (lib/view_selection.cc:14-161; bundle may be NULL: position-based).
 * A view whose `bytes` is NULL has no image in the embedding; width <= 0
 * marks a hole in the view list (a null View::Ptr).  out: room for n_views
 * indices; *n_out receives how many were written. */
int smvs_host_select_neighbors(const smvs_host_view *views, int n_views,
    const smvs_host_bundle *bundle, int view, int num_neighbors, int *out,
    int *n_out);

/* smvs_amd::BlockStencilMatrix::multiply (BlockSparseMatrix<4>::multiply,
 * lib/block_sparse_matrix.h:276-298) on the host, no device involved:
 * y = A x for the block stencil blocks9[num_nodes][9][16]. */
int smvs_host_block_multiply(int num_nodes, int node_stride, const double *blocks9,
    const double *x, double *y);

#ifdef __cplusplus
}
#endif
#endif
