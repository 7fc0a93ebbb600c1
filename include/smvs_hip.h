/*
 * smvs_hip.h -- C ABI of the MI355X (gfx950) depth-optimisation hot path.
 *
 * This is the drop-in boundary: a host DepthOptimizer (ours in
 * smvs_amd/csrc/host/, or the reference's lib/depth_optimizer.cc with the
 * binding shown in INTEGRATION.md) calls these entry points instead of
 * GaussNewtonStep / ConjugateGradient / Surface::update_nodes /
 * LightOptimizer / SGMStereo.  file:line citations are relative to the
 * flanggut/smvs tree and name the reference interface each entry replaces.
 *
 * Conventions
 *  - every function returns 0 (SMVS_OK) or a negative smvs_status; nothing
 *    throws; smvs_last_error() gives the text of the last failure of the
 *    calling thread.  The reference throws std::invalid_argument on
 *    dimension mismatch (block_sparse_matrix.h:136-138, sse_vector.cc:22-23,
 *    conjugate_gradient.h:77-78): the host wrapper re-throws from the status.
 *  - pointers are caller-owned HOST memory unless the name ends in _dev.
 *  - images use MVE's layout: interleaved channels, row-major,
 *    index (y*W + x)*C + c.
 *  - one context is used by one host thread at a time; different contexts
 *    may be used concurrently (one reference view per context, as the
 *    reference's one-task-per-view pool, app/smvsrecon.cc:658-733).
 *  - a context owns its device buffers and one HIP stream.
 */
#ifndef SMVS_HIP_H
#define SMVS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct smvs_ctx smvs_ctx;

typedef enum {
    SMVS_OK = 0,
    SMVS_ERR_INVALID = -1,   /* bad argument / dimension mismatch */
    SMVS_ERR_HIP = -2,       /* HIP runtime error (see smvs_last_error) */
    SMVS_ERR_STATE = -3,     /* call order violated (e.g. solve before construct) */
    SMVS_ERR_NOMEM = -4
} smvs_status;

/* ConjugateGradient::ReturnInfo, conjugate_gradient.h:22-27 */
typedef enum {
    SMVS_CG_CONVERGENCE = 0,
    SMVS_CG_MAX_ITERATIONS = 1,
    SMVS_CG_INVALID_INPUT = 2
} smvs_cg_info;

#define SMVS_MAX_SUBS 16

const char *smvs_last_error(void);
/* Number of HIP devices visible (0 when none / no driver). */
int smvs_device_count(void);

/* ------------------------------------------------------------------ */
/* context                                                            */
/* ------------------------------------------------------------------ */

/* One reference view (StereoView main + n_subs neighbours,
 * depth_optimizer.h:48-51).  width/height = main view size. */
int smvs_ctx_create(int device, int width, int height, int n_subs,
    smvs_ctx **out);
/* Parks the context (its device buffers and stream stay allocated) for the
 * next smvs_ctx_create of the same device / size / neighbour count: a view's
 * few hundred MB are not returned to the driver between views.
 * smvs_release_workspaces() frees the parked contexts. */
int smvs_ctx_destroy(smvs_ctx *ctx);
int smvs_ctx_synchronize(smvs_ctx *ctx);

/* Which implementation of ConjugateGradient::solve (conjugate_gradient.h:72-202)
 * the context uses -- not in the reference, which has one.  All of them run
 * the same preconditioned CG with the same termination rules (:136-198):
 *   AUTO          the fastest one that applies: the chip-resident solver when
 *                 the node grid fits the chip (<= 256 tiles of <= 512 nodes),
 *                 with ONE grid-wide exchange per iteration (eight dot
 *                 products of the current vectors are reduced before the
 *                 step length is known; r.r, z.r, x.(b + r) of the updated
 *                 vectors follow from them one step ahead); otherwise the
 *                 streaming kernels
 *   STREAMING     assembly kernel + two launches per iteration (csrc/cg.hip);
 *                 any grid size
 *   RESIDENT_REF  the chip-resident solver with the reference's operation
 *                 order: d.Ad first, then r.r, z.r, x.(b + r) of the updated
 *                 vectors (two exchanges per iteration); falls back to
 *                 STREAMING when the grid does not fit
 * A mode that cannot run (co-residency lost, grid too large) degrades to
 * STREAMING; the choice never changes results beyond the summation order. */
typedef enum {
    SMVS_SOLVER_AUTO = 0,
    SMVS_SOLVER_STREAMING = 1,
    SMVS_SOLVER_RESIDENT_REF = 2
} smvs_solver_mode;
int smvs_ctx_set_solver(smvs_ctx *ctx, int mode);

/* DepthOptimizer::prepare_correspondences, depth_optimizer.cc:679-699:
 * Mi[n_subs][9] row-major and ti[n_subs][3], already widened from the float
 * CameraInfo::fill_reprojection result; flen / inv_flen =
 * StereoView::get_flen / get_inverse_flen (stereo_view.h:132-148). */
int smvs_ctx_set_cameras(smvs_ctx *ctx, const double *Mi, const double *ti,
    float flen, float inv_flen);

/* Per-scale planes of the main view, StereoView::get_image_gradients /
 * get_shading_image / get_shading_gradients (stereo_view.h:43-47).
 * shading / shading_grad may be NULL (no -S). */
int smvs_ctx_upload_main(smvs_ctx *ctx, const float *grad2,
    const float *shading1, const float *shading_grad2);
/* Per-scale planes of neighbour `sub`: get_image_gradients (2 ch) and
 * get_image_hessian (3 ch: I_xx, I_xy, I_yy), stereo_view.cc:167-187. */
int smvs_ctx_upload_sub(smvs_ctx *ctx, int sub, int width, int height,
    const float *grad2, const float *hess3);

/* Scale space on the device: what StereoView's constructor
 * and StereoView::set_scale compute on the host (stereo_view.cc:16-46, 97-188).
 * smvs_ctx_upload_image stores the u8 image of the main view (view = -1) or of
 * neighbour `view` (interleaved channels, 1 or 3).  smvs_ctx_set_scale then
 * produces, for every view with an image, the gradient / Hessian planes of
 * that scale (byte -> float, Gaussian blur with sigma = 0.12 * 2^scale + 0.2,
 * luminance, 3x3 quadratic fit) directly in the context: nothing crosses PCIe
 * per scale.  smvs_ctx_download_planes hands planes back to host-side
 * topology code; hess3 may be NULL (the main view keeps no Hessian). */
int smvs_ctx_upload_image(smvs_ctx *ctx, int view, int width, int height,
    int channels, const uint8_t *bytes);
/* The same without waiting for the transfer (StereoView::create x 9 at the
 * start of a view's task, app/smvsrecon.cc:662-691, costs the reference
 * nothing on the device; here it is 56 MB over PCIe): with `bytes` in
 * page-locked memory (smvs_pinned_alloc) the DMA is enqueued on a copy stream
 * of the context and the call returns at once; the byte -> float conversion
 * runs where the image is first needed (smvs_ctx_set_scale converts view by
 * view, so a view's blur and gradients overlap the next views' transfers).
 * `bytes` must stay valid and unchanged until smvs_ctx_synchronize / the
 * context's destruction.  Pageable memory: identical to smvs_ctx_upload_image. */
int smvs_ctx_upload_image_async(smvs_ctx *ctx, int view, int width, int height,
    int channels, const uint8_t *bytes);
int smvs_ctx_set_scale(smvs_ctx *ctx, int scale);
int smvs_ctx_download_planes(smvs_ctx *ctx, int view, float *grad2,
    float *hess3);
/* shading image + gradients alone (scale independent, stereo_view.cc:64-84) */
int smvs_ctx_upload_shading(smvs_ctx *ctx, const float *shading1,
    const float *shading_grad2);
/* The same planes made on the device from the main view's uploaded image:
 * StereoView::initialize_linear (lib/stereo_view.cc:64-84) -- the inverse sRGB
 * curve per element, the luminance (0.21, 0.72, 0.07) and rows x and y of the
 * 3x3 quadratic fit of the unblurred image -- in place of the host's loops and
 * smvs_ctx_upload_shading, bit for bit.  gamma_lut256: the curve at the 256
 * values (float)k / 255.0f an image element can take, evaluated by the caller
 * with the host's own expression (the device evaluates no powf); NULL: no
 * gamma correction.  Needs the main image (smvs_ctx_upload_image[_async] with
 * view = -1; SMVS_ERR_INVALID without one); an upload still on its way is
 * converted first.  Only enqueues on the context's stream.
 * smvs_ctx_download_shading hands the planes back, whichever entry made them
 * (either pointer may be NULL; SMVS_ERR_STATE when there are none). */
int smvs_ctx_prepare_shading(smvs_ctx *ctx, const float *gamma_lut256);
int smvs_ctx_download_shading(smvs_ctx *ctx, float *shading1,
    float *shading_grad2);

/* Surface state (surface.h:106-120) as flat arrays.
 *   nodes[(npx+1)*(npy+1)][4] = f, dx, dy, dxy (patch units);
 *   node_valid / patch_valid: non-null node / patch;
 *   patch_vis[p] bit j <=> j in subsurfaces[p] (depth_optimizer.h:108).
 * Resets the active set to "all valid nodes" (depth_optimizer.cc:204-212). */
int smvs_ctx_set_surface(smvs_ctx *ctx, int scale, int npx, int npy,
    int start_x, int start_y, const double *nodes, const uint8_t *node_valid,
    const uint8_t *patch_valid, const uint32_t *patch_vis);
/* active_nodes (std::vector<char>, depth_optimizer.cc:205); NULL = all valid */
int smvs_ctx_set_active(smvs_ctx *ctx, const uint8_t *active);
int smvs_get_active(smvs_ctx *ctx, uint8_t *active, int *num_active);
int smvs_get_nodes(smvs_ctx *ctx, double *nodes);
int smvs_set_nodes(smvs_ctx *ctx, const double *nodes);
/* Device-resident copy of the nodes (not in the reference, whose surface lives
 * in host memory): save keeps the current nodes in HBM, restore brings them
 * back on the context's stream without a transfer -- a caller that reruns the
 * optimisation from one start (bench.py, parameter sweeps) uploads it once.
 * restore without a save, or after smvs_ctx_set_surface changed the grid,
 * returns SMVS_ERR_STATE. */
int smvs_ctx_save_nodes(smvs_ctx *ctx);
int smvs_ctx_restore_nodes(smvs_ctx *ctx);
/* A second context that holds everything the Newton loop of `src` reads at
 * this moment -- cameras, the scale's gradient / Hessian planes of all views,
 * the surface (nodes, validity, visibility masks), the lighting -- copied on
 * the device, with its nodes saved (smvs_ctx_restore_nodes).  Not in the
 * reference: it is how bench.py keeps the start state of every Newton batch of
 * one DepthOptimizer::optimize (lib/depth_optimizer.cc:219-304 is entered 15
 * times per view) resident in HBM and replays exactly those loops as its timed
 * region.  The clone is an ordinary context (smvs_ctx_destroy). */
int smvs_ctx_clone_loop_state(smvs_ctx *src, smvs_ctx **out);

/* ------------------------------------------------------------------ */
/* Gauss-Newton step                                                  */
/* ------------------------------------------------------------------ */

/* GaussNewtonStep::construct, gauss_newton_step.cc:33-143, with
 * GaussNewtonStep::Options {regularization, light_surf_regularization}
 * (gauss_newton_step.h:28-34); lighting16 = GlobalLighting::Params or NULL.
 * H, g, P stay on the device.  num_active_patches (may be NULL) = patches
 * with at least one active node (gauss_newton_step.cc:73-79). */
int smvs_gn_construct(smvs_ctx *ctx, double regularization,
    double light_surf_regularization, const double *lighting16,
    int *num_active_patches);

/* Test / parity hooks: download the assembled system.  H9[n][s][16]: 4x4
 * row-major block (row node n, col node n + dy*(npx+1) + dx), slot
 * s = (dy+1)*3 + dx+1; zero where the reference holds no block.
 * g[4n+k]; P[n][16] inverted diagonal blocks.  Any pointer may be NULL. */
int smvs_gn_download(smvs_ctx *ctx, double *H9, double *g, double *P);
/* per-patch 16x16 systems and 16-gradients before assembly
 * (sub_hessian / sub_gradient, gauss_newton_step.cc:61-62); entries of
 * patches that were not evaluated are unspecified.  The device keeps the
 * upper triangle (the part the assembly reads, gauss_newton_step.cc:103,
 * 113-119); the lower one comes back as its mirror. */
int smvs_gn_download_patch_systems(smvs_ctx *ctx, double *Hp, double *gp);
/* Overwrite the assembled system (solver tests on arbitrary systems). */
int smvs_gn_upload(smvs_ctx *ctx, const double *H9, const double *g,
    const double *P);

/* ConjugateGradient::solve, conjugate_gradient.h:72-202, on b = -g with the
 * block-Jacobi preconditioner, x0 = 0.  error_tolerance < 0 selects the
 * optimizer's rule error_tolerance = 0.01 * ||g|| (depth_optimizer.cc:247).
 * num_iterations / info as ConjugateGradient::Status. */
int smvs_cg_solve(smvs_ctx *ctx, int max_iterations, double error_tolerance,
    double q_tolerance, int *num_iterations, int *info);
int smvs_cg_download_x(smvs_ctx *ctx, double *x);
int smvs_cg_upload_x(smvs_ctx *ctx, const double *x);

/* depth_optimizer.cc:267-303: NaN guard on delta[0], fill_node_reprojections,
 * Surface::update_nodes (surface.cc:957-981), fill_node_reprojections, then
 * either the mean reprojection delta (full_optimization) or the new active
 * set (node active if any pixel of an incident patch moved by more than
 * `threshold` = 0.15).  When nan_flag is set nothing was updated. */
int smvs_update_and_reactivate(smvs_ctx *ctx, double threshold,
    int full_optimization, int *num_active, double *mean_delta,
    int *nan_flag);

/* The whole Newton loop of one outer iteration, depth_optimizer.cc:204-304:
 * four launches per step, no host round trip inside a step, and the next step
 * is enqueued before the previous one has ended (the loop condition of
 * :219-220 / :267-268 / :284-288 is evaluated on the device).
 * The call returns when the loop has ended and the stream is idle.  Between
 * the call's steps nothing is materialised for smvs_gn_download (H, g, P live
 * in registers); smvs_cg_download_x holds the last step's delta. */
typedef struct {
    double regularization;             /* DepthOptimizer::Options */
    double light_surf_regularization;
    int full_optimization;
    int max_newton_steps;              /* 200, depth_optimizer.cc:219 */
    int cg_max_iterations;             /* 200, :246 */
    double cg_q_tolerance;             /* 1e-3, conjugate_gradient.h:34 */
    double active_threshold;           /* 0.15, :296 */
    double full_opt_threshold;         /* 0.01, :285 */
    int use_lighting;                  /* lighting != nullptr */
    double lighting[16];
    int reset_active;                  /* 1: start from all valid nodes */
} smvs_gn_loop_params;

typedef struct {
    int newton_steps;
    int linear_iterations;             /* sum of CG iterations, :257 */
    long long active_patch_steps;      /* sum over steps of active patches */
    int final_active_nodes;
    int nan_break;                     /* loop left through :267-268 */
} smvs_gn_loop_stats;

int smvs_gn_run_loop(smvs_ctx *ctx, const smvs_gn_loop_params *params,
    smvs_gn_loop_stats *stats);

/* ------------------------------------------------------------------ */
/* surface outputs + lighting                                         */
/* ------------------------------------------------------------------ */

/* Surface::get_depth_map / get_normal_map, surface.cc:155-183 (float
 * images, zero where no patch). depth[W*H], normals[W*H*3]. */
int smvs_get_depth_map(smvs_ctx *ctx, float *depth);
int smvs_get_normal_map(smvs_ctx *ctx, float *normals);

/* Both maps in one pass over the surface (one kernel, two transfers, one
 * synchronisation) -- the end of DepthOptimizer::optimize,
 * depth_optimizer.cc:150-160.  inv_calibration9 != NULL: the depth map comes
 * back as StereoView::write_depth_to_view stores it (stereo_view.h:100-119:
 * MVE's ray-length convention, depth times the length of the pixel's viewing
 * ray under CameraInfo::fill_inverse_calibration); NULL: z-depth, as
 * smvs_get_depth_map. */
int smvs_get_maps(smvs_ctx *ctx, const float *inv_calibration9, float *depth,
    float *normals);

/* Page-locked host memory for the large buffers that cross the boundary (the
 * views' u8 images, the 33 MB of depth + normal maps per 1920x1080 view): a
 * transfer from / to such a buffer is one DMA at link rate, a pageable buffer
 * goes through a staging copy on the host (3-4 ms per view at 1920x1080 x 9).
 * Not in the reference, whose images live in pageable mve::Image storage; any
 * pointer works everywhere, pinned ones are just faster.  Buffers are pooled
 * by size (page-locking costs more than the copy it saves) and go back to the
 * driver with smvs_release_workspaces(). */
int smvs_pinned_alloc(size_t bytes, void **out);
int smvs_pinned_free(void *ptr);

/* LightOptimizer::fit_lighting_to_image accumulation,
 * light_optimizer.cc:32-49, over the uploaded shading image: A[16][16],
 * b[16] (the 16x16 pseudo inverse stays on the host).  The _dev variant
 * leaves 272 doubles (A then b) in a device buffer for an optional RCCL
 * all-reduce ("shared lighting" extension) and returns its
 * device pointer. */
int smvs_light_accumulate(smvs_ctx *ctx, double *A256, double *b16);
int smvs_light_accumulate_dev(smvs_ctx *ctx, double **Ab272_dev);
/* Reads the context's 272-double buffer back (after the caller's collective
 * has summed it in place over the views that share their lighting). */
int smvs_light_download(smvs_ctx *ctx, double *A256, double *b16);
/* The other direction: puts normal equations into the context's buffer -- sums
 * a caller has kept (a lock-step round continued later), or a known pattern
 * (bench.py checks the RCCL all-reduce of smvs_rccl.h with one). */
int smvs_light_upload(smvs_ctx *ctx, const double *A256, const double *b16);

/* ------------------------------------------------------------------ */
/* SGM                                                                */
/* ------------------------------------------------------------------ */

/* SGMStereo::run_sgm, sgm_stereo.cc:98-124, for one (main, neighbour)
 * pair of u8 images already at SGM scale (sgm_stereo.cc:31-39):
 * census cost volume over num_steps inverse-depth planes, 8-path
 * aggregation (constant P2, the SSE branch :361-406), WTA.
 * M[9], t[3]: float reprojection main -> neighbour at SGM resolution
 * (sgm_stereo.cc:154-160).  Outputs (any may be NULL):
 *   depth[w*h]  (sgm_stereo.cc:274-306),
 *   argmin[w*h] winning plane index,
 *   cost[w*h*num_steps], sgm[w*h*num_steps] u16 volumes (parity tests).
 * Plane counts: num_steps is 2 .. 128, or a multiple of 8 from 136 to 256;
 * any other count is SMVS_ERR_INVALID before any device call.  Why 8:
 * SGMStereo::Options::num_steps is a free integer, but the reference's default
 * build (SMVS_ENABLE_SSE, lib/defines.h:21) aggregates in groups of eight
 * planes (sgm_stereo.cc:355-356, 377, 399, 416) and is only defined for
 * multiples of eight; the counts up to 128 stay as they were.  Why 256: the
 * winner-takes-all key keeps the plane index in one byte.  The bytes above
 * 128 planes are the reference's, as below; a 960 x 540 x 256 run holds
 * 133 MB of warped and of cost bytes each and 1.06 GB of path bytes. */
int smvs_sgm_run(int device, const uint8_t *main_img, int w, int h,
    const uint8_t *neighbor_img, int nw, int nh, const float *M,
    const float *t, float min_depth, float max_depth, int num_steps,
    uint16_t penalty1, uint16_t penalty2, float *depth, int32_t *argmin,
    uint16_t *cost, uint16_t *sgm);

/* The whole SGM initialisation of one reference view on the device:
 * reconstruct_sgm_depth_for_view, app/smvsrecon.cc:346-384, i.e. for each of
 * the first one or two neighbours SGMStereo::reconstruct (sgm_stereo.cc:46-96:
 * run_sgm main -> neighbour, run_sgm neighbour -> main, left/right
 * consistency check :64-91 with integer pixel coordinates, 3 % border and
 * depth ratio 0.8) and the merge of the two checked maps (:366-377).  The
 * four cost volumes, the depth maps and the check never leave the device;
 * only the merged z-depth map (w*h floats) is copied back.
 * Images: u8, one channel, already at SGM scale (SGMStereo's constructor,
 * sgm_stereo.cc:27-39).  M_fwd / t_fwd: CameraInfo::fill_reprojection main ->
 * neighbour at the two SGM image sizes (also the matrix of the check, :56-62);
 * M_bwd / t_bwd: neighbour -> main.  range_main / range_neighbor: {min, max}
 * depth of the two runs (SGMStereo::fill_depth_range_for_view, :669-720, or
 * the caller's fixed range). */
typedef struct {
    const uint8_t *image;
    int width, height;
    float M_fwd[9], t_fwd[3];
    float M_bwd[9], t_bwd[3];
    float range_main[2];
    float range_neighbor[2];
} smvs_sgm_neighbor;

/* num_steps: the plane counts of smvs_sgm_run (2 .. 128, or a multiple of 8
 * from 136 to 256: the reference's default build is defined for multiples of
 * eight only), used by all four runs of the view; any other count is
 * SMVS_ERR_INVALID before any device call. */
int smvs_sgm_depth_for_view(int device, const uint8_t *main_img, int w, int h,
    const smvs_sgm_neighbor *neighbors, int n_neighbors, int num_steps,
    uint16_t penalty1, uint16_t penalty2, float *depth);

/* The same with SGMStereo's constructor (sgm_stereo.cc:27-39) on the device as
 * well: the images are the views' FULL-resolution u8 embeddings (interleaved,
 * `channels` / neighbor_channels[k] = 1 or 3); StereoView::get_byte_image
 * (desaturate<uint8_t>, stereo_view.cc:86-95) and `halvings` x
 * mve::image::rescale_half_size run on the device.  w, h and the neighbours'
 * width / height are the full-resolution sizes; the reprojections, the depth
 * ranges and the output map refer to the SGM-scale sizes ((s + 1) >> 1 per
 * halving).  num_steps: as for smvs_sgm_depth_for_view. */
int smvs_sgm_depth_for_view_raw(int device, const uint8_t *main_img, int w, int h,
    int channels, const smvs_sgm_neighbor *neighbors, const int *neighbor_channels,
    int n_neighbors, int halvings, int num_steps, uint16_t penalty1,
    uint16_t penalty2, float *depth);

/* Which of the reference's two path aggregations the three entries above
 * reproduce.  The reference selects it at build time (SMVS_ENABLE_SSE,
 * lib/defines.h):
 *   SMVS_SGM_P2_CONSTANT  the SSE build, sgm_stereo.cc:361-406: constant
 *                         penalty2 (what the entries without `_mode` run);
 *   SMVS_SGM_P2_ADAPTIVE  the build without SSE, sgm_stereo.cc:310-346: per
 *                         (pixel, predecessor on the path)
 *                         penalty2' = max(penalty1 * 3 / 2, penalty2 / (|I - I'| + 1))
 *                         in int, I = the u8 main image at SGM scale; and, as
 *                         that build does (:626-654), the two bottom corners
 *                         start their upward diagonal with 2 C.
 * Mode 0 gives the bytes of the entry without `_mode`.  An unknown mode -- and
 * penalties for which a wrap of the u16 volumes cannot be excluded,
 * 8 * (255 + max(penalty2, penalty1 * 3 / 2)) + 4 * 255 >= 65536 -- is
 * SMVS_ERR_INVALID before any device call.  penalty2 < penalty1 is accepted in
 * the adaptive mode (penalty2' >= penalty1 always) and refused in mode 0.
 * The plane counts are those of smvs_sgm_run in both modes. */
typedef enum { SMVS_SGM_P2_CONSTANT = 0, SMVS_SGM_P2_ADAPTIVE = 1 } smvs_sgm_p2_mode;

/* smvs_sgm_run with the aggregation of sgm_stereo.cc:310-346 selectable */
int smvs_sgm_run_mode(int device, const uint8_t *main_img, int w, int h,
    const uint8_t *neighbor_img, int nw, int nh, const float *M,
    const float *t, float min_depth, float max_depth, int num_steps,
    uint16_t penalty1, uint16_t penalty2, int p2_mode, float *depth,
    int32_t *argmin, uint16_t *cost, uint16_t *sgm);
/* smvs_sgm_depth_for_view with the aggregation of sgm_stereo.cc:310-346
 * selectable (all four runs of a view use the mode, each with its own main
 * image: the neighbour's in the neighbour -> main runs) */
int smvs_sgm_depth_for_view_mode(int device, const uint8_t *main_img, int w, int h,
    const smvs_sgm_neighbor *neighbors, int n_neighbors, int num_steps,
    uint16_t penalty1, uint16_t penalty2, int p2_mode, float *depth);
/* smvs_sgm_depth_for_view_raw with the aggregation of sgm_stereo.cc:310-346
 * selectable (the image of the penalty is the desaturated, halved one) */
int smvs_sgm_depth_for_view_raw_mode(int device, const uint8_t *main_img, int w, int h,
    int channels, const smvs_sgm_neighbor *neighbors, const int *neighbor_channels,
    int n_neighbors, int halvings, int num_steps, uint16_t penalty1,
    uint16_t penalty2, int p2_mode, float *depth);

/* Which depth the winner-takes-all step of a run stores.  Not in the reference:
 * depth_from_sgm_volume (sgm_stereo.cc:274-306) returns the depth of the
 * winning plane, so a map holds at most num_steps - 2 distinct values.
 *   SMVS_SGM_WINNER_PLANE     that (what every entry above runs);
 *   SMVS_SGM_WINNER_SUBPLANE  the parabola through the aggregated cost S of the
 *                             winner i (the first minimum, as before) and of
 *                             its two neighbours refines it.  All in float, in
 *                             this order, no contraction, IEEE division:
 *     inv[0] = 1.0f / max_depth, inc = (1.0f / min_depth - inv[0]) / (num_steps - 1),
 *     inv[k + 1] = inv[k] + inc          (sgm_stereo.cc:197-203: the planes'
 *                                         depths are 1.0f / inv[k])
 *     a = S[i - 1], b = S[i], c = S[i + 1] as int, den = a - 2 b + c   (>= 0)
 *     off = 0 if i == num_steps - 1 or den == 0,
 *           else (float)(a - c) / (float)(2 * den)                    (|off| <= 0.5)
 *     n = i + 1 if off > 0, else i - 1
 *     depth = 1.0f / (inv[i] + fabsf(off) * (inv[n] - inv[i]))
 *                             With off == 0 that is the plane's depth to the
 *                             bit.  argmin stays i, and the rule of
 *                             sgm_stereo.cc:300-303 (no depth for i < 2 and
 *                             for main_img < 25) is unchanged, as are the
 *                             left/right check and the merge behind it.
 * p2_mode: smvs_sgm_p2_mode, as in the `_mode` entries.  A NULL options
 * pointer or an unknown winner is SMVS_ERR_INVALID before any device call, as
 * are an unknown p2_mode, the plane counts and the penalties; { p2_mode,
 * SMVS_SGM_WINNER_PLANE } gives the bytes of the `_mode` entry. */
typedef enum { SMVS_SGM_WINNER_PLANE = 0, SMVS_SGM_WINNER_SUBPLANE = 1 } smvs_sgm_winner;
typedef struct { int p2_mode; int winner; } smvs_sgm_options;

/* smvs_sgm_run_mode with the winner of sgm_stereo.cc:274-306 selectable */
int smvs_sgm_run_opts(int device, const uint8_t *main_img, int w, int h,
    const uint8_t *neighbor_img, int nw, int nh, const float *M,
    const float *t, float min_depth, float max_depth, int num_steps,
    uint16_t penalty1, uint16_t penalty2, const smvs_sgm_options *opts, float *depth,
    int32_t *argmin, uint16_t *cost, uint16_t *sgm);
/* smvs_sgm_depth_for_view_mode with the winner of sgm_stereo.cc:274-306
 * selectable (all four runs of a view, sgm_stereo.cc:46-62, use it; the check
 * of :64-91 and the merge of app/smvsrecon.cc:366-377 see the refined maps) */
int smvs_sgm_depth_for_view_opts(int device, const uint8_t *main_img, int w, int h,
    const smvs_sgm_neighbor *neighbors, int n_neighbors, int num_steps,
    uint16_t penalty1, uint16_t penalty2, const smvs_sgm_options *opts, float *depth);
/* smvs_sgm_depth_for_view_raw_mode with the winner of sgm_stereo.cc:274-306
 * selectable */
int smvs_sgm_depth_for_view_raw_opts(int device, const uint8_t *main_img, int w, int h,
    int channels, const smvs_sgm_neighbor *neighbors, const int *neighbor_channels,
    int n_neighbors, int halvings, int num_steps, uint16_t penalty1,
    uint16_t penalty2, const smvs_sgm_options *opts, float *depth);

/* How the checked maps of a view's neighbours become one map.  The reference
 * (app/smvsrecon.cc:360-377) looks at the first two neighbours only and
 * averages them where both have a depth:
 *   SMVS_SGM_MERGE_REFERENCE  that: one or two neighbours, the bytes of the
 *                             `_opts` entries (min_agree and agree_ratio are
 *                             not read);
 *   SMVS_SGM_MERGE_CONSENSUS  not in the reference: n = 1 .. SMVS_MAX_SUBS
 *                             neighbours, 2 n runs, and per pixel the largest
 *                             group of maps that agree with one of them.
 * Definition of the consensus.  Per pixel, c[0 .. n-1] are the left/right-
 * checked forward depths of the n neighbours in neighbour order (the check is
 * sgm_stereo.cc:64-91, unchanged; 0 means no depth).  All arithmetic in float,
 * in this order, no contraction, IEEE division:
 *     best = 0, best_count = 0
 *     for k = 0 .. n-1 with c[k] != 0:
 *         count = number of j in 0 .. n-1 with c[j] != 0 and
 *                 (j == k  or  fminf(c[j], c[k]) / fmaxf(c[j], c[k]) >= agree_ratio)
 *         if count > best_count: best_count = count, best = k
 *                                       (strict: ties keep the lowest k)
 *     if best_count == 0 or best_count < min_agree: out = 0
 *     else: s = 0.0f
 *           for j ascending over the supporters of c[best] (the set counted
 *               above): s = s + c[j]
 *           out = s / (float)best_count
 * The supporters are taken around one candidate (a star), not as a transitive
 * closure: with a ~ b ~ c and a !~ c, b's star holds all three and a's two.
 * support[pixel] = best_count as u8 (also where out = 0 because of min_agree).
 * Two consequences hold to the bit: n = 2, agree_ratio = 0, min_agree = 1 gives
 * the reference merge's bytes ((a + b) / 2.0f == (a + b) * 0.5f), and n = 1,
 * min_agree = 1 gives the checked map itself.
 * Accepted: n in 1 .. SMVS_MAX_SUBS, agree_ratio in [0, 1], min_agree in
 * 1 .. SMVS_MAX_SUBS; anything else (a NaN ratio, a NULL options pointer, an
 * unknown merge or winner, three neighbours with the reference's merge) is
 * SMVS_ERR_INVALID before any device call.
 * agree_ratio = 0.95 and min_agree = 2 are what the host mirror and the Python
 * layer default to.  They are defaults of a user option, not tuned values: at
 * 128 planes over a 3 .. 12 range adjacent planes differ by 0.6 % at the near
 * end and by 2.4 % at the far end, so 0.95 admits about two planes at the far
 * end (the left/right check uses 0.8).  Nobody has measured their effect on
 * real scenes. */
typedef enum { SMVS_SGM_MERGE_REFERENCE = 0, SMVS_SGM_MERGE_CONSENSUS = 1 } smvs_sgm_merge;
typedef struct {
    int p2_mode;        /* smvs_sgm_p2_mode */
    int winner;         /* smvs_sgm_winner */
    int merge;          /* smvs_sgm_merge */
    int min_agree;
    float agree_ratio;
} smvs_sgm_view_options;

/* smvs_sgm_depth_for_view_opts / _raw_opts with the merge selectable.  With
 * the consensus the neighbour images are prepared one at a time, the n forward
 * and n backward maps stay on the device, and one kernel does the n left/right
 * checks and the merge per pixel.  Optional outputs of the consensus (NULL:
 * not wanted; with the reference's merge they must be NULL):
 *   checked[n * w * h]  the n checked forward maps, neighbour-major,
 *   support[w * h]      best_count.
 * (w, h of the outputs: the SGM-scale size, as for depth.) */
int smvs_sgm_depth_for_view_merge(int device, const uint8_t *main_img, int w, int h,
    const smvs_sgm_neighbor *neighbors, int n_neighbors, int num_steps,
    uint16_t penalty1, uint16_t penalty2, const smvs_sgm_view_options *opts,
    float *depth, float *checked, uint8_t *support);
int smvs_sgm_depth_for_view_raw_merge(int device, const uint8_t *main_img, int w, int h,
    int channels, const smvs_sgm_neighbor *neighbors, const int *neighbor_channels,
    int n_neighbors, int halvings, int num_steps, uint16_t penalty1,
    uint16_t penalty2, const smvs_sgm_view_options *opts, float *depth, float *checked,
    uint8_t *support);

/* The check-and-merge kernel alone, on maps of the caller (as smvs_sgm_run
 * exposes one run): fwd[n * w * h] are the n unchecked forward maps of the main
 * view, neighbors[k] holds neighbour k's own backward map bwd[width * height]
 * and the float reprojection main -> neighbour of the check.  opts: merge must
 * be SMVS_SGM_MERGE_CONSENSUS (p2_mode and winner are not read).  Outputs, any
 * may be NULL: merged[w * h], checked[n * w * h], support[w * h].  A
 * correspondence that is not a number fails the check. */
typedef struct {
    const float *bwd;
    int width, height;
    float M_fwd[9], t_fwd[3];
} smvs_sgm_check_neighbor;
int smvs_sgm_check_merge(int device, const float *fwd, int w, int h,
    const smvs_sgm_check_neighbor *neighbors, int n_neighbors,
    const smvs_sgm_view_options *opts, float *merged, float *checked, uint8_t *support);

/* Multi-neighbour plane sweep.  Not in the reference, and not a value of
 * smvs_sgm_merge: instead of 2 n runs and a merge of n depth maps, ONE cost
 * volume of the main view from all n neighbours, aggregated once, one winner.
 * All n forward runs of a view share its pixel grid, its census and its depth
 * planes (the main view's depth range does not depend on the neighbour,
 * sgm_stereo.cc:50-57), so per view the work is n x (warp + cost), one fold,
 * one path aggregation, one WTA.  Integers only.
 *
 * Definition.  c[k][p][d] is the cost byte of neighbour k, k = 0 .. n-1 in
 * neighbour order, at pixel p and plane d: the byte create_cost_volume
 * (sgm_stereo.cc:192-244) gives for the pair (main, neighbour k) over the main
 * view's planes.  A byte of 255 is no cost; any other byte is a cost.
 * Fold, per (p, d), in int:
 *     m = number of k with c[k] != 255
 *     if m < min_views:            C = 255
 *     else: k_eff = (best_k == 0) ? m : min(best_k, m)
 *           S = sum of the k_eff smallest c[k] != 255   (a multiset: ties need no order)
 *           C = (2 * S + k_eff) / (2 * k_eff)           (integer division: mean, half up)
 * Two consequences hold to the byte: n = 1 with min_views = 1 gives c[0], and
 * j copies of one neighbour give that neighbour's volume for any best_k.  The
 * intermediates fit 16 bits (2 * 254 * 16 + 16 < 65536).
 * Run.  aggregate_sgm_costs and depth_from_sgm_volume run on C exactly as on the
 * volume of a pair, for either p2_mode and either winner; the rule of
 * sgm_stereo.cc:300-303 (no depth for a winner index below 2 or a main-image
 * byte below 25), the depth table and the bound on the penalties are unchanged.
 * There is no neighbour-side run and no left/right check.
 * Support, per pixel with winner plane i:
 *     support = number of k with c[k][p][i] <= support_cost      (u8)
 * If min_support > 0 and support < min_support, depth is 0; argmin stays i.
 * Accepted: n in 1 .. SMVS_MAX_SUBS, min_views in 1 .. n, best_k in
 * 0 .. SMVS_MAX_SUBS, support_cost in 0 .. 254, min_support in 0 .. n,
 * 0 < min_depth < max_depth, the plane counts and penalties of
 * smvs_sgm_run_opts; anything else (a NULL options pointer, an unknown p2_mode
 * or winner) is SMVS_ERR_INVALID before any device call.
 * min_views = min(2, n), best_k = (n + 1) / 2, support_cost = 20 and
 * min_support = min(2, n) are what the host mirror and the Python layer default
 * to: defaults of a user option, untuned; nobody has measured them on real
 * scenes.
 * Memory: the n volumes of w * h * num_steps bytes are all held until the
 * support kernel has run (a slot of the pooled workspace, next to the volumes
 * of one run): 66 MB each at 960 x 540 x 128, and 2.1 GB for n = 16 at
 * 960 x 540 x 256. */
typedef struct {
    int p2_mode;        /* smvs_sgm_p2_mode */
    int winner;         /* smvs_sgm_winner */
    int min_views;
    int best_k;
    int support_cost;
    int min_support;
} smvs_sgm_sweep_options;

/* The sweep for one view, images at SGM scale (u8, one channel).  Of
 * neighbors[k] only image, width, height, M_fwd and t_fwd are read; range[2] =
 * { min_depth, max_depth } of the main view.  A neighbour image may be as small
 * as 2 x 2 (it is never a main view).  Outputs, any may be NULL: depth[w * h],
 * argmin[w * h], support[w * h], cost[w * h * num_steps] (u16: the folded
 * volume C), sgm[w * h * num_steps] (u16, as smvs_sgm_run gives it). */
int smvs_sgm_sweep_for_view(int device, const uint8_t *main_img, int w, int h,
    const smvs_sgm_neighbor *neighbors, int n_neighbors, const float *range, int num_steps,
    uint16_t penalty1, uint16_t penalty2, const smvs_sgm_sweep_options *opts, float *depth,
    int32_t *argmin, uint8_t *support, uint16_t *cost, uint16_t *sgm);
/* The same on the views' full-resolution u8 embeddings, desaturated and halved
 * on the device as in smvs_sgm_depth_for_view_raw (sizes, reprojections and
 * outputs as there).  Outputs, either may be NULL: depth, support. */
int smvs_sgm_sweep_for_view_raw(int device, const uint8_t *main_img, int w, int h, int channels,
    const smvs_sgm_neighbor *neighbors, const int *neighbor_channels, int n_neighbors,
    int halvings, const float *range, int num_steps, uint16_t penalty1, uint16_t penalty2,
    const smvs_sgm_sweep_options *opts, float *depth, uint8_t *support);
/* The fold kernel alone, on bytes of the caller (as smvs_sgm_check_merge exposes
 * the consensus kernel): costs[n_neighbors * len], neighbour-major, out[len];
 * len in 1 .. 2^32.  min_views and best_k as above. */
int smvs_sgm_fold_costs(int device, const uint8_t *costs, int n_neighbors, size_t len,
    int min_views, int best_k, uint8_t *out);

/* Two single-run rejections for the front end above.  Not in the reference;
 * both off by default, and with both off every entry below gives the bytes and
 * the launches of the entry it extends.
 *
 * Uniqueness test.  Integers only.  Per pixel of a run, after the winner i has
 * been found (the first minimum, unchanged), with S the aggregated u16 sums,
 * b = S[i] and D = num_steps:
 *     competitors = { d in 0 .. D-1 : |d - i| > uniqueness_window }
 *     if competitors is empty:  the pixel passes;  runner_up = 65535
 *     else  r = min over competitors of S[d];      runner_up = r
 *           rejected  iff  r * (100 - uniqueness) < b * 100     (int, 32 bits)
 * A rejected pixel gets depth 0; argmin stays i; the rule of
 * sgm_stereo.cc:300-303 is unchanged, and the sub-plane winner computes what it
 * computed for a pixel that passes.  The comparison is strict: a competitor
 * exactly at the bound passes.  The test is part of the WTA step of EVERY run
 * of an entry, the neighbour-side runs of a view included.  uniqueness = 0
 * rejects nothing and launches the WTA kernels of the entries above.
 * uniqueness in 0 .. 99 (a percentage), uniqueness_window in 1 .. 256 (planes).
 * The window is an option because the usual fixed +-1 assumes planes a pixel
 * apart: at 128 planes over depths 3 .. 12 adjacent planes are less than a
 * pixel apart and window 1 rejects half of a synthetic pair's valid pixels,
 * window 16 a twentieth.  The defaults of the layers above (0, 1) are defaults
 * of a user option, untuned; nobody has measured them on real scenes.
 *
 * Speckle removal.  On a depth map of w x h floats:
 *     a pixel is valid iff depth > 0.0f (a NaN is not);
 *     two valid 4-neighbours (x +- 1 or y +- 1) a, b are linked iff
 *         fminf(a, b) / fmaxf(a, b) >= speckle_ratio   (IEEE division, no
 *         contraction: the idiom of the consensus);
 *     components are the transitive closure of the links (unlike the
 *         consensus's star, a ~ b ~ c puts a and c together);
 *     size[p] = the number of pixels of p's component as u32, 0 for a pixel
 *         that is not valid;
 *     out[p] = 0 where 0 < size[p] < speckle_size, else the input's bits.
 * The partition is a fact of the input, so the result is defined to the bit.
 * speckle_size 0 and 1 remove nothing (off: no launch); speckle_ratio in
 * [0, 1].  The filter runs on the final map of a view, before the download:
 * after the reference merge, after the consensus merge (checked and support
 * stay those of the merge), after the sweep's support test.  Its launches are
 * timed in class SMVS_SGM_K_MERGE of smvs_sgm_profile.
 *
 * SMVS_ERR_INVALID before any device call: a NULL filter pointer, uniqueness
 * outside 0 .. 99, a window outside 1 .. 256, a negative speckle_size, a ratio
 * outside [0, 1] or NaN, speckle_size > 1 on the run entry, a runner_up output
 * with uniqueness = 0. */
typedef struct {
    int uniqueness;
    int uniqueness_window;
    int speckle_size;
    float speckle_ratio;
} smvs_sgm_filter_options;

/* smvs_sgm_run_opts with the uniqueness test; extra optional output
 * runner_up[w * h] (u16).  The speckle fields must be off. */
int smvs_sgm_run_filtered(int device, const uint8_t *main_img, int w, int h,
    const uint8_t *neighbor_img, int nw, int nh, const float *M,
    const float *t, float min_depth, float max_depth, int num_steps,
    uint16_t penalty1, uint16_t penalty2, const smvs_sgm_options *opts,
    const smvs_sgm_filter_options *filter, float *depth, int32_t *argmin, uint16_t *cost,
    uint16_t *sgm, uint16_t *runner_up);
/* smvs_sgm_depth_for_view_merge / _raw_merge with the filters */
int smvs_sgm_depth_for_view_filtered(int device, const uint8_t *main_img, int w, int h,
    const smvs_sgm_neighbor *neighbors, int n_neighbors, int num_steps,
    uint16_t penalty1, uint16_t penalty2, const smvs_sgm_view_options *opts,
    const smvs_sgm_filter_options *filter, float *depth, float *checked, uint8_t *support);
int smvs_sgm_depth_for_view_raw_filtered(int device, const uint8_t *main_img, int w, int h,
    int channels, const smvs_sgm_neighbor *neighbors, const int *neighbor_channels,
    int n_neighbors, int halvings, int num_steps, uint16_t penalty1,
    uint16_t penalty2, const smvs_sgm_view_options *opts,
    const smvs_sgm_filter_options *filter, float *depth, float *checked, uint8_t *support);
/* smvs_sgm_sweep_for_view / _raw with the filters; extra optional output of the
 * first: runner_up[w * h] (u16) */
int smvs_sgm_sweep_for_view_filtered(int device, const uint8_t *main_img, int w, int h,
    const smvs_sgm_neighbor *neighbors, int n_neighbors, const float *range, int num_steps,
    uint16_t penalty1, uint16_t penalty2, const smvs_sgm_sweep_options *opts,
    const smvs_sgm_filter_options *filter, float *depth, int32_t *argmin, uint8_t *support,
    uint16_t *cost, uint16_t *sgm, uint16_t *runner_up);
int smvs_sgm_sweep_for_view_raw_filtered(int device, const uint8_t *main_img, int w, int h,
    int channels, const smvs_sgm_neighbor *neighbors, const int *neighbor_channels,
    int n_neighbors, int halvings, const float *range, int num_steps, uint16_t penalty1,
    uint16_t penalty2, const smvs_sgm_sweep_options *opts,
    const smvs_sgm_filter_options *filter, float *depth, uint8_t *support);
/* The 18 view and sweep entries (14 above, the two with the photo test and the
 * two with the refinement sweeps below) are three front ends behind one call record (csrc/sgm_internal.h,
 * SgmViewCall): an entry fixes the fields it does not take and hands on the
 * rest.  "SGM scale": channels = 1 for the main image
 * and every neighbour, halvings = 0.  "constant, plane": p2_mode =
 * SMVS_SGM_P2_CONSTANT, winner = SMVS_SGM_WINNER_PLANE.  "off": both filters off
 * (uniqueness = 0, speckle_size = 0), no runner_up.  Every entry but the last two
 * also fixes the photo test: off (radius 0), no witness, no confidence, no views.
 * Every entry but the two `_refine` ones fixes the refinement sweeps: off
 * (sweeps 0), no slant.
 *
 *   entry                                 front                 fixes
 *   smvs_sgm_depth_for_view               reference merge       SGM scale; constant, plane; off
 *   smvs_sgm_depth_for_view_mode          reference merge       SGM scale; plane; off
 *   smvs_sgm_depth_for_view_opts          reference merge       SGM scale; off
 *   smvs_sgm_depth_for_view_raw           reference merge       constant, plane; off
 *   smvs_sgm_depth_for_view_raw_mode      reference merge       plane; off
 *   smvs_sgm_depth_for_view_raw_opts      reference merge       off
 *   smvs_sgm_depth_for_view_merge         opts->merge: either   SGM scale; off
 *   smvs_sgm_depth_for_view_filtered      opts->merge: either   SGM scale
 *   smvs_sgm_depth_for_view_raw_merge     opts->merge: either   off
 *   smvs_sgm_depth_for_view_raw_filtered  opts->merge: either   nothing
 *   smvs_sgm_sweep_for_view               plane sweep           SGM scale; off
 *   smvs_sgm_sweep_for_view_filtered      plane sweep           SGM scale
 *   smvs_sgm_sweep_for_view_raw           plane sweep           off; no argmin, cost, sgm
 *   smvs_sgm_sweep_for_view_raw_filtered  plane sweep           no argmin, cost, sgm, runner_up
 *   smvs_sgm_depth_for_view_raw_photo     opts->merge: either   nothing
 *   smvs_sgm_sweep_for_view_raw_photo     plane sweep           nothing
 *   smvs_sgm_depth_for_view_raw_refine    opts->merge: either   nothing
 *   smvs_sgm_sweep_for_view_raw_refine    plane sweep           nothing
 *
 * The reference merge has the depth map as its only output (checked and support
 * must be NULL); the consensus adds checked and support; the sweep's outputs
 * are all optional.  All 18 make their argument checks in one order, before
 * any device call (csrc/sgm_view.hip, check_sgm_view_call). */

/* Multi-view photo-consistency test.  Not in the reference; opt-in, off by
 * default (radius 0), and with it off the two entries below give the bytes and
 * the launches of the `_filtered` entries.  A depth of the view's final map is
 * kept only where the main image around the pixel, warped at that depth, agrees
 * with the best few of n witness images; the same kernel gives a per-pixel
 * confidence.  The definition is normative (tests/sgm_photo_ref.py restates it).
 *
 * Inputs: the main image I (u8, w x h, one channel, at SGM scale); a depth map a
 * of w x h floats in the depth convention of the SGM planes (what every front
 * end produces); n witnesses (1 <= n <= 16), each a u8 image of nw x nh and the
 * float reprojection M[9], t[3] main -> witness; radius r in 1 .. 3
 * (N = (2 r + 1)^2), best_k (0: all), min_views, min_score.
 *
 * A pixel is valid iff a > 0.0f (a NaN is not: the speckle filter's rule).  A
 * pixel that is not valid keeps its bits and gets confidence -1.0f and views 0.
 *
 * For a valid pixel (x, y) and a witness k, j = -r .. r (outer), i = -r .. r
 * (inner):
 *     xc = clamp(x + i, 0, w - 1), yc = clamp(y + j, 0, h - 1), A = I[yc][xc];
 *     (B, inside) = the sample of warped_neighbors_for_depth
 *         (sgm_stereo.cc:163-188) for main pixel (xc, yc) at THE CENTRE PIXEL'S
 *         depth a(x, y), evaluated as the warp kernel of the runs evaluates it:
 *         float, contraction off, px = 0.5f + xc, py = 0.5f + yc, the three-term
 *         sums from 0.0f, p = (M (px, py, 1)) * a + t, two IEEE divisions by
 *         p2, - 0.5f, the u8 linear_at with + 0.5f.  One difference: inside is
 *         stated positively,
 *             inside = !(p2 < 0) && p0 >= 0 && p1 >= 0 && p0 <= nw - 1
 *                      && p1 <= nh - 1,
 *         so a coordinate that is not a number is outside; for every other input
 *         this is the reference's test;
 *     integer sums: SA += A, SB += B, SAB += A B, SAA += A A, SBB += B B (all
 *         below 2^31 for r <= 3).
 * Witness k is defined iff all N samples were inside.  Then
 *     cov = N SAB - SA SB,  va = N SAA - SA^2,  vb = N SBB - SB^2,
 *     score_k = 0.0 if va == 0 || vb == 0 (a flat window is no evidence), else
 *     score_k = (double)(cov |cov|) / (double)(va vb):
 * both products are exact integers below 2^53, the score is one IEEE double
 * division: the signed squared correlation in [-1, 1].  (Not the NCC itself, on
 * purpose: no square root, so nothing but correctly rounded + - x / decides a
 * bit.)
 * Per pixel, with c the number of defined witnesses and
 * k' = min(best_k ? best_k : n, c):
 *     confidence = -1.0f if c < max(min_views, 1), else
 *         (float)((s_1 + s_2 + ... + s_k') / (double)k'), the defined scores in
 *         descending order, added in that order in double;
 *     out = 0.0f where confidence < min_score (a float comparison: a pixel
 *         exactly at the bound is kept), else the input's bits;
 *     views = c as u8.
 * min_score = -1 drops nothing (confidence only).
 *
 * In the two view entries `neighbors` (and neighbor_channels) hold
 * n_neighbors + n_witness entries, at most 16: the first n_neighbors go through
 * the front exactly as in the `_filtered` entry, ALL of them are witnesses (of a
 * witness behind n_neighbors only image, width, height, M_fwd and t_fwd are
 * read).  Every image is uploaded and prepared once per call.  The test runs on
 * the final map of the view, before the speckle removal; checked and support
 * stay those of the unfiltered map.  One launch, timed in class
 * SMVS_SGM_K_MERGE of smvs_sgm_profile.  The defaults of the layers above
 * (radius 0, best_k 2, min_views 2, min_score 0.49) are defaults of a user
 * option, untuned; nobody has measured them on real scenes.
 *
 * SMVS_ERR_INVALID before any device call, behind the checks of the `_filtered`
 * entry and in this order: a NULL photo pointer; radius outside 0 .. 3; best_k
 * or min_views outside 0 .. n_neighbors + n_witness; min_score outside [-1, 1]
 * or NaN; n_witness < 0 or more than 16 entries in all; with radius 0 a
 * witness, a confidence or a views output (an error, never silently ignored);
 * a witness without an image, with a size below 1 x 1 at SGM scale or with a
 * channel count other than 1 or 3. */
typedef struct { int radius; int best_k; int min_views; float min_score; } smvs_sgm_photo_options;

/* smvs_sgm_depth_for_view_raw_filtered with the test; extra optional outputs
 * confidence[w * h] (f32) and views[w * h] (u8) at SGM scale. */
int smvs_sgm_depth_for_view_raw_photo(int device, const uint8_t *main_img, int w, int h,
    int channels, const smvs_sgm_neighbor *neighbors, const int *neighbor_channels,
    int n_neighbors, int halvings, int num_steps, uint16_t penalty1,
    uint16_t penalty2, const smvs_sgm_view_options *opts,
    const smvs_sgm_filter_options *filter, float *depth, float *checked, uint8_t *support,
    int n_witness, const smvs_sgm_photo_options *photo, float *confidence, uint8_t *views);
/* smvs_sgm_sweep_for_view_filtered on raw images (every optional output of it)
 * with the test */
int smvs_sgm_sweep_for_view_raw_photo(int device, const uint8_t *main_img, int w, int h,
    int channels, const smvs_sgm_neighbor *neighbors, const int *neighbor_channels,
    int n_neighbors, int halvings, const float *range, int num_steps, uint16_t penalty1,
    uint16_t penalty2, const smvs_sgm_sweep_options *opts,
    const smvs_sgm_filter_options *filter, float *depth, int32_t *argmin, uint8_t *support,
    uint16_t *cost, uint16_t *sgm, uint16_t *runner_up, int n_witness,
    const smvs_sgm_photo_options *photo, float *confidence, uint8_t *views);
/* The kernel alone, on a map and SGM-scale images of the caller: main_img
 * [w * h], depth[w * h], out[w * h] (may be depth itself), confidence[w * h] and
 * views[w * h] (either may be NULL); of a witness only image, width, height,
 * M_fwd and t_fwd are read.  No minimum size; w * h < 2^31 for every image.
 * radius in 1 .. 3, n in 1 .. 16, the other options as above. */
int smvs_sgm_photo_check(int device, const uint8_t *main_img, int w, int h, const float *depth,
    const smvs_sgm_neighbor *witnesses, int n, const smvs_sgm_photo_options *opts, float *out,
    float *confidence, uint8_t *views);

/* Multi-view plane refinement sweeps.  Not in the reference; opt-in, off by
 * default (sweeps 0), and with them off the two `_refine` entries below give the
 * bytes and the launches of the `_photo` entries.  The photo test's confidence
 * becomes an objective: every pixel holds a small plane hypothesis (a depth and
 * two slants), and red-black sweeps let it adopt a 4-neighbour's extrapolated
 * plane, or a deterministic perturbation of its own, whenever that raises its
 * confidence.  The definition is normative (tests/sgm_refine_ref.py restates
 * it); it extends the block above and uses its vocabulary.
 *
 * Inputs: those of the photo test (I, a, n witnesses, smvs_sgm_photo_options
 * with radius 1 .. 3) and smvs_sgm_refine_options: sweeps in 0 .. 8 (0: off),
 * samples in 0 .. 8, depth_step and slant_step finite in [0, 1], seed, fill 0 or 1.
 *
 * Hypothesis.  A pixel has none, or (a, gx, gy), three floats with a > 0.  The
 * depth of window sample (i, j), i, j = -r .. r, is
 *     d = a + gx * (float)i;  d = d + gy * (float)j;
 * two rounded products and two rounded sums in this order, contraction off.
 * Linear in depth, not in inverse depth, on purpose: with gx = gy = 0 every
 * sample depth is a's bits.
 *
 * Confidence of a hypothesis at (x, y): the photo test's confidence with "the
 * centre pixel's depth" replaced by d(i, j) per sample.  A sample with !(d > 0)
 * counts as outside (the witness is then not defined).  The integer sums, the
 * score, the mean of the best k' in descending order in double, the cast to
 * float, -1.0f with fewer than max(min_views, 1) defined witnesses and views = c
 * are unchanged.
 *
 * Start.  A pixel valid in the input (a > 0.0f) has (a, 0, 0) with that
 * hypothesis's confidence and views: exactly the photo test's.  Every other pixel
 * has no hypothesis, confidence -1.0f and views 0.
 *
 * Sweep t = 0 .. sweeps - 1, half-sweep c = 0, 1.  Active are the pixels with
 * ((x + y) & 1) == c; with fill = 0 only those valid in the input.  An active
 * pixel considers the candidates below in this order; a candidate replaces the
 * pixel's hypothesis, confidence and views iff its confidence, as a float, is
 * strictly greater than the current one (a tie keeps the earlier; a pixel without
 * a hypothesis holds -1.0f).
 *   1. The left (x - 1), right (x + 1), up (y - 1) and down (y + 1) neighbour, if
 *      it is inside the image and has a hypothesis (a', gx', gy').  The slants
 *      are taken over; the depth is extrapolated by one float addition:
 *          left a' + gx',  right a' - gx',  up a' + gy',  down a' - gy';
 *      skipped if !(depth > 0).  The four neighbours have the other colour and do
 *      not change in this half-sweep, so working in place is race-free and the
 *      result does not depend on the launch geometry.
 *   2. m = 0 .. samples - 1, only if the pixel has a hypothesis (a, gx, gy) by
 *      then, each from the pixel's hypothesis AT THAT MOMENT, all in uint32:
 *          mix(v): v ^= v >> 16; v *= 0x7feb352d; v ^= v >> 15; v *= 0x846ca68b;
 *                  v ^= v >> 16;
 *          h0  = mix(seed ^ mix((uint32)(y * w + x) ^ mix((uint32)(t * 16 + m))));
 *          h_j = mix(h0 + j * 0x9e3779b9), j = 1, 2, 3;
 *          u_j = (float)((int32)(h_j >> 8) - 8388608) * 2^-23   (exact, [-1, 1));
 *          s = 2^-t (exact);
 *          e = a * depth_step;  e = e * s;  a" = a + e * u_1;
 *          g = a * slant_step;  g = g * s;  gx" = gx + g * u_2;  gy" = gy + g * u_3;
 *      every product and sum rounded, contraction off; skipped if !(a" > 0).
 *
 * End.  A pixel with a hypothesis: out = 0.0f where confidence < min_score (the
 * photo test's float comparison), else out = a; slant = (gx, gy); confidence and
 * views those of the final hypothesis (a dropped pixel keeps all three).  A pixel
 * without a hypothesis keeps its input bits (NaN and negatives included),
 * confidence -1.0f, views 0, slant (0, 0).
 *
 * Consequences: sweeps = 0 gives the photo test's three outputs to the byte and
 * zero slants; a pixel valid in the input never ends with a lower confidence
 * than the photo test gives it; fill = 0 never gives a depth to a pixel that had
 * none.
 *
 * In the two view entries the refinement takes the photo test's place: on the
 * view's final map, before the speckle removal; checked and support stay those
 * of the unfiltered map.  1 + 2 sweeps + 1 launches, timed in class
 * SMVS_SGM_K_MERGE of smvs_sgm_profile.  The defaults of the layers above (sweeps
 * 0, samples 2, depth_step 0.02, slant_step 0.01, seed 1, fill 1; at 128 planes
 * over 3 .. 12 two planes are about 2 % apart at the far end) are defaults of a
 * user option, untuned; nobody has measured them on real scenes.
 *
 * SMVS_ERR_INVALID before any device call, behind the checks of the `_photo`
 * entry and in this order: a NULL refine pointer; sweeps or samples outside
 * 0 .. 8; depth_step or slant_step outside [0, 1] or NaN; fill other than 0 or 1;
 * sweeps > 0 with photo radius 0; a slant output with sweeps 0 (errors, never
 * silently ignored). */
typedef struct {
    int sweeps; int samples; float depth_step; float slant_step; uint32_t seed; int fill;
} smvs_sgm_refine_options;

/* smvs_sgm_depth_for_view_raw_photo with the sweeps; extra optional output
 * slant[h][w][2] (f32, gx then gy) at SGM scale. */
int smvs_sgm_depth_for_view_raw_refine(int device, const uint8_t *main_img, int w, int h,
    int channels, const smvs_sgm_neighbor *neighbors, const int *neighbor_channels,
    int n_neighbors, int halvings, int num_steps, uint16_t penalty1,
    uint16_t penalty2, const smvs_sgm_view_options *opts,
    const smvs_sgm_filter_options *filter, float *depth, float *checked, uint8_t *support,
    int n_witness, const smvs_sgm_photo_options *photo, float *confidence, uint8_t *views,
    const smvs_sgm_refine_options *refine, float *slant);
/* smvs_sgm_sweep_for_view_raw_photo with the sweeps */
int smvs_sgm_sweep_for_view_raw_refine(int device, const uint8_t *main_img, int w, int h,
    int channels, const smvs_sgm_neighbor *neighbors, const int *neighbor_channels,
    int n_neighbors, int halvings, const float *range, int num_steps, uint16_t penalty1,
    uint16_t penalty2, const smvs_sgm_sweep_options *opts,
    const smvs_sgm_filter_options *filter, float *depth, int32_t *argmin, uint8_t *support,
    uint16_t *cost, uint16_t *sgm, uint16_t *runner_up, int n_witness,
    const smvs_sgm_photo_options *photo, float *confidence, uint8_t *views,
    const smvs_sgm_refine_options *refine, float *slant);
/* The kernels alone, on a map and SGM-scale images of the caller, as
 * smvs_sgm_photo_check: out[w * h] (may be depth itself), slant[w * h * 2],
 * confidence[w * h] and views[w * h] (each of the three may be NULL).  No minimum
 * size; radius in 1 .. 3, n in 1 .. 16; sweeps = 0 is accepted (the start and the
 * end alone: the photo test's outputs and zero slants). */
int smvs_sgm_plane_refine(int device, const uint8_t *main_img, int w, int h, const float *depth,
    const smvs_sgm_neighbor *witnesses, int n, const smvs_sgm_photo_options *photo,
    const smvs_sgm_refine_options *refine, float *out, float *slant, float *confidence,
    uint8_t *views);

/* The speckle kernels alone, on a map of the caller: depth[w * h], out[w * h]
 * (may be depth itself), size[w * h] (may be NULL); w * h < 2^31.  The kernels
 * run for every speckle_size (0 and 1 give the input's bits and the sizes). */
int smvs_sgm_filter_speckles(int device, const float *depth, int w, int h, int speckle_size,
    float speckle_ratio, float *out, uint32_t *size);

/* DepthOptimizer::depthmap_bilateral_filter, depth_optimizer.cc:957-1004 */
int smvs_bilateral_upsample(int device, const float *dm, int dm_w, int dm_h,
    const float *ci, int w, int h, int channels, float sigma,
    int kernel_size, float *out);

/* The same filter inside a view's context (DepthOptimizer::create_initial_surface,
 * depth_optimizer.cc:35-51: init = depthmap_bilateral_filter(sgm_depth,
 * main_view->get_image())): guided by the main image smvs_ctx_upload_image
 * left on the device (SMVS_ERR_STATE without one), result written to
 * out[W*H] (may be NULL) AND kept in the context as the SGM depth map the
 * visibility tests of smvs_topology_subviews compare with -- the reference
 * hands the same filtered map to both (:41-45, :463-466).  dm == NULL forgets
 * the resident map. */
int smvs_ctx_sgm_init_depth(smvs_ctx *ctx, const float *dm, int dm_w, int dm_h,
    float sigma, int kernel_size, float *out);

/* The same with the map as the view stores it: dm_mve[dm_w*dm_h] is the
 * "smvs-sgm" embedding in MVE's ray-length convention
 * (StereoView::write_depth_to_view, stereo_view.h:100-119) and
 * inv_calibration9 the inverse calibration of an image of the map's size
 * (StereoView::get_sgm_depth, stereo_view.h:121-135:
 * mve::image::depthmap_convert_conventions(depth, invproj, false)).  The
 * conversion to z-depth runs on the device with the host's float operations
 * (same bits); a caller that would otherwise convert 0.5 M pixels on the host
 * while the GPU waits for the map calls this one (create_initial_surface,
 * depth_optimizer.cc:35-45).  dm_is_z_depth != 0: dm is still the z-depth map
 * the SGM front end produced (reconstruct_sgm_depth_for_view,
 * app/smvsrecon.cc:346-384) and has not been stored yet: the kernel applies
 * write_depth_to_view's conversion (`dm *= len`) and then get_sgm_depth's
 * (`dm *= 1.0 / len`) -- the round trip through the embedding the reference
 * makes, same bits, without the host touching 2 x 0.5 M pixels. */
int smvs_ctx_sgm_init_depth_mve(smvs_ctx *ctx, const float *dm, int dm_w, int dm_h,
    const float *inv_calibration9, int dm_is_z_depth, float sigma, int kernel_size, float *out);

/* ------------------------------------------------------------------ */
/* topology tests between Newton batches              */
/* ------------------------------------------------------------------ */

/* The per-(patch, neighbour) part of DepthOptimizer::create_subview_surfaces,
 * depth_optimizer.cc:433-590, for the surface of smvs_ctx_set_surface and the
 * images of smvs_ctx_upload_image: z-buffer of the surface depth map (and of
 * sgm_depth[W*H]; NULL: the map smvs_ctx_sgm_init_depth left in the context,
 * if any, else none; the reference splats it when use_sgm is set, :463-466)
 * in every neighbour, then border / occlusion test (:505-530),
 * warp anisotropy <= 8 (:532-575) and, if use_ncc (the reference's !use_sgm,
 * :577-580), ncc_for_patch >= 0 (:792-912).
 * patch_vis_out[num_patches] (may be NULL: nothing is copied back): bit j =
 * patch visible in neighbour j; 0 for invalid patches.  The mask also becomes
 * the context's patch visibility.
 * Deleting the patches without any neighbour (:592-603) stays with the
 * caller, which owns the topology. */
int smvs_topology_subviews(smvs_ctx *ctx, const float *sgm_depth, int use_ncc,
    uint32_t *patch_vis_out);

/* DepthOptimizer::mse_for_patch, depth_optimizer.cc:747-790, for every valid
 * patch with the visibility set by smvs_ctx_set_surface: mean gradient
 * mismatch against the visible neighbours (1.0 without any); -1 for invalid
 * patches.  cut_boundaries (:360-431) thresholds it at 0.05. */
int smvs_topology_patch_mse(smvs_ctx *ctx, double *mse_out);

/* The `while (deleted > 10) cut_boundaries()` loops of the optimiser
 * (depth_optimizer.cc:186-190, 323-337; cut_boundaries :360-431) on the
 * surface of smvs_ctx_set_surface (incl. its visibility masks): every pass
 * deletes patches with a depth discontinuity (:371-399) and patches that have
 * a node with more than one missing neighbour node and mse_for_patch > 0.05
 * (:401-428), then nodes without a patch (Surface::remove_nodes_without_patch).
 * inv_calibration9: CameraInfo::fill_inverse_calibration of the main view.
 * patch_valid_out[num_patches], node_valid_out[num_nodes] (either may be NULL:
 * not copied back): validity after the last pass (also the context's);
 * *total_deleted (may be NULL). */
int smvs_topology_cut_boundaries(smvs_ctx *ctx, const float *inv_calibration9,
    uint8_t *patch_valid_out, uint8_t *node_valid_out, int *total_deleted);

/* ------------------------------------------------------------------ */
/* grid surgery of the surface on the device          */
/* ------------------------------------------------------------------ */

/* smvs::Surface's topology operations (lib/surface.h:36-57) on the surface the
 * context holds, so that DepthOptimizer::optimize (depth_optimizer.cc:53-162)
 * never moves the surface across PCIe between its Newton batches.  The grid
 * geometry follows the reference's integer rules (surface.cc:28-37, 983-1012)
 * and is mirrored on the host by smvs_surface_info; node values are the
 * reference's double arithmetic in its operation order.  Every call leaves the
 * number of valid (non-null) patches in *num_valid_patches (may be NULL) --
 * the one quantity the optimiser's outer loop needs (:339-356) -- and resets
 * the visibility masks when the grid changed.  A call that is asked for no
 * count (every output pointer NULL) only ENQUEUES its kernels on the
 * context's stream and returns without waiting for the device: the sequence
 * between two Newton batches costs one synchronisation, with its last call. */
typedef struct {
    int scale, patchsize;      /* patchsize = 2^scale */
    int npx, npy;              /* patches; nodes = (npx + 1) * (npy + 1) */
    int start_x, start_y;      /* pixel of node (0, 0) */
} smvs_surface_geometry;

/* Surface::create, surface.cc:19-53: the grid of `scale` with its nodes
 * initialised from a depth map (initialize_node_from_depth :667-760 for every
 * node, fill_holes :630-651, remove_nodes_without_patch :762-869).  The map --
 * Surface::depth, kept in the context for the fill_patches_from_depth calls
 * that follow every subdivision (depth_optimizer.cc:97-106) -- is
 *   depth != NULL                  depth[W*H], positive = valid (:74-79);
 *   depth == NULL, n_points > 0    zero except the listed pixels: the bundle's
 *                                  features projected into the view by the
 *                                  caller (initialize_depth_from_bundle
 *                                  :90-130), at most one entry per pixel;
 *   depth == NULL, n_points == 0   the filtered SGM map that
 *                                  smvs_ctx_sgm_init_depth left in the context
 *                                  (create_initial_surface,
 *                                  depth_optimizer.cc:41-45). */
int smvs_surface_create(smvs_ctx *ctx, int scale, const float *depth,
    const int32_t *point_pixel, const float *point_depth, int n_points,
    int *num_valid_patches);
/* Surface::fill_patches_from_depth, surface.cc:140-152 */
int smvs_surface_fill_patches_from_depth(smvs_ctx *ctx, int *num_valid_patches);
/* Surface::subdivide_patches, surface.cc:983-1107: scale - 1, five new nodes
 * per patch (a later patch overwrites an earlier one's edge midpoints, as the
 * reference's loop does), old nodes with rescaled derivatives, then
 * fill_holes + remove_nodes_without_patch. */
int smvs_surface_subdivide(smvs_ctx *ctx, int *num_valid_patches);
/* Surface::expand, surface.cc:482-628: two rounds of extrapolated border
 * nodes (check_swap_nodes :472-480), fill_holes, remove_nodes_without_patch.
 * *num_filled (may be NULL) = its return value, the patches filled. */
int smvs_surface_expand(smvs_ctx *ctx, int *num_filled, int *num_valid_patches);
/* Surface::remove_isolated_patches, surface.cc:887-927 (the in-place,
 * column-by-column walk reproduced exactly) + remove_nodes_without_patch. */
int smvs_surface_remove_isolated_patches(smvs_ctx *ctx, int *num_valid_patches);
/* The tail of create_subview_surfaces, depth_optimizer.cc:592-603: patches
 * whose visibility mask (smvs_topology_subviews) is empty are deleted, then
 * remove_nodes_without_patch. */
int smvs_surface_delete_unseen_patches(smvs_ctx *ctx, int *num_deleted,
    int *num_valid_patches);
/* Test hook of the scripted sequences (tests/test_host_surface_cpu.py runs the
 * same scripts on the host mirror): deletes every `every`-th valid patch in
 * id order, then remove_nodes_without_patch. */
int smvs_surface_delete_every(smvs_ctx *ctx, int every, int *num_valid_patches);
/* Geometry of the context's surface (either pointer may be NULL). */
int smvs_surface_info(smvs_ctx *ctx, smvs_surface_geometry *geometry,
    int *num_valid_patches);
/* The arrays of smvs_ctx_set_surface back on the host (any may be NULL):
 * nodes[(npx+1)*(npy+1)][4], node_valid, patch_valid, patch_vis. */
int smvs_surface_download(smvs_ctx *ctx, double *nodes, uint8_t *node_valid,
    uint8_t *patch_valid, uint32_t *patch_vis);

/* Node slopes from the SGM plane hypotheses.  Not in the reference; opt-in, and
 * without the three entries below every entry gives the bytes and the launches
 * it gave before.  initialize_node_from_depth (surface.cc:667-760) sets a
 * node's dx, dy, dxy from differences of the quadrant minima of its window: on
 * a plane of slope b per pixel two quadrants ps/2 apart differ by b ps/2, while
 * the bicubic patch (bicubic_patch.cc:20-86, Hermite on the unit square) needs
 * dx = b ps -- half the slope, a dxy made of noise, a one-sided difference next
 * to a hole.  The slants of the `_refine` entries above are the missing datum.
 * The definition is normative (tests/surface_planes_ref.py restates it).
 *
 * Slant plane of a context.  Inputs: L, the resident SGM-scale z-depth map
 * (dm_w x dm_h, what smvs_ctx_sgm_init_depth[_mve] left behind its upload
 * kernel's conversion), and G = slant[dm_h][dm_w][2], z-depth per SGM pixel, gx
 * then gy, as `_refine` writes it.  With the bilateral's factors
 *     scale_x = (float)dm_w / (float)W;  scale_y = (float)dm_h / (float)H;
 * the full-resolution pixel (x, y) reads the bilateral's centre tap
 * (depth_optimizer.cc:981-984)
 *     sx = (int)clamp(scale_x * (float)x, 0.f, (float)dm_w - 1.f);  sy likewise.
 * If L(sx, sy) > 0.0f and both components of G(sx, sy) are finite,
 *     P(x, y) = (G(sx, sy, 0) * scale_x, G(sx, sy, 1) * scale_y),
 * one rounded float product each, contraction off; otherwise both components are
 * the quiet NaN 0x7FC00000: "no slant".  P is W x H x 2 f32, z-depth per
 * full-resolution pixel.
 *
 * Node from its window, with slants.  The window is the reference's: four
 * quadrants of (ps/2)^2 pixels.  Its statistics -- the count of positive
 * depths, the quadrant minima, the median -- are unchanged, and they alone
 * decide whether the node exists and what f is.  In addition S is the set of
 * window pixels inside the image with D > 0 and both components of P finite,
 * cs = |S|.  With cs == 0 the node's dx, dy, dxy are the reference's.  With
 * cs >= 1, mx is the element of 0-based rank cs / 2 of { P(p, 0) : p in S } in
 * ascending key order (the rule f follows), my the same for component 1, taken
 * independently, where
 *     key(v) = bits ^ 0x80000000 if the sign bit is clear, else ~bits
 * (so -0.0 < +0.0: the choice is a fact of the multiset, not of the traversal),
 * and
 *     dx = (double)mx * (double)ps;  dy = (double)my * (double)ps;  dxy = 0.0.
 *
 * Consequences: node_valid, patch_valid and every f are the bytes of the
 * slant-free run; an all-NaN plane gives the slant-free nodes to the byte. */

/* The slant plane P of the context from slant[dm_h][dm_w][2]; call it after
 * smvs_ctx_sgm_init_depth[_mve].  SMVS_ERR_STATE without a resident map,
 * SMVS_ERR_INVALID when dm_w x dm_h is not that map's size.  P stays in the
 * context; out[W*H*2] (may be NULL) receives it.  slant == NULL forgets P, and
 * so does every call of smvs_ctx_sgm_init_depth[_mve] (a new map invalidates
 * it).  P is not part of smvs_ctx_clone_loop_state. */
int smvs_ctx_sgm_init_slants(smvs_ctx *ctx, const float *slant, int dm_w, int dm_h,
    float *out);
/* smvs_surface_create with the rule above.  depth[W*H] and slant[W*H*2] (a
 * plane P) are either both the caller's or both NULL; both NULL: the resident
 * ones (SMVS_ERR_STATE if either is missing).  The surface keeps the plane as
 * it keeps Surface::depth: the smvs_surface_fill_patches_from_depth calls that
 * follow every subdivision use the same rule for the null nodes, until
 * smvs_surface_create ends that.  Enqueue-only when no count is asked for. */
int smvs_surface_create_planes(smvs_ctx *ctx, int scale, const float *depth,
    const float *slant, int *num_valid_patches);
/* The plane the surface holds, out[W*H*2] (SMVS_ERR_STATE without one). */
int smvs_surface_slants(smvs_ctx *ctx, float *out);

/* ------------------------------------------------------------------ */
/* consumer of the depth / normal maps                */
/* ------------------------------------------------------------------ */

/* MeshGenerator::cut_depth_maps, mesh_generator.cc:24-158, with the normal
 * preparation of generate_mesh (:189-208) and ViewProjection (:300-342): the
 * cross-view consistency cut over all views at once.
 *   depth   : width*height floats, MVE convention (ray length) as stored by
 *             StereoView::write_depth_to_view (the "smvs-B<scale>" embedding);
 *             overwritten with the cut map ("smvs-cut", :229)
 *   normals : width*height*3 floats, camera space as DepthOptimizer writes
 *             them ("smvs-B<scale>N"); overwritten with the world-space normals
 *             (:199-207), which the point export reads afterwards
 *   flen / rot / trans : mve::CameraInfo (world -> camera)
 * With a single view only the normals are transformed (:211). */
typedef struct {
    int width, height;
    float flen;
    float rot[9], trans[3];
    float *depth;
    float *normals;
} smvs_mesh_view;

int smvs_cut_depth_maps(int device, smvs_mesh_view *views, int n_views);

/* The point cloud of MeshGenerator::generate_mesh, mesh_generator.cc:160-299
 * (the default path of smvsrecon, app/smvsrecon.cc:278-343): per view
 * DepthTriangulator::full_triangulation (mve::geom::depthmap_triangulate),
 * depthmap_mesh_confidences(m, 4), the scale value (:252-262) and the normal
 * lookup (:264-276), merged in view-list order; optionally clipped to an AABB
 * (smvsrecon.cc:306-319).  The semantics pinned for the MVE pieces are the
 * [MVE-unverified] table of DESIGN.md section 9.
 *   depth / normals : as smvs_mesh_view, but read only
 *   image           : width*height*channels bytes (the colour embedding at
 *                     the depth map's size; 1 channel = grey)
 *   cut_depth       : optional out (may be NULL): the map that was
 *                     triangulated -- the "smvs-cut" embedding (:222-226)
 *                     when cutting, else the input depth */
typedef struct {
    int width, height;
    float flen;
    float rot[9], trans[3];
    const float *depth;
    const float *normals;
    const uint8_t *image;
    int channels;
    float *cut_depth;
} smvs_point_view;

typedef struct {
    int cut_surfaces;     /* MeshGenerator::Options::cut_surfaces (--no-cut: 0) */
    int use_aabb;         /* --aabb: delete vertices outside [aabb_min, aabb_max] */
    float aabb_min[3], aabb_max[3];
    float dd_factor;      /* depthmap_triangulate's discontinuity factor, 5 */
    int want_faces;       /* keep the triangles for smvs_points_download (tests);
                             not available together with use_aabb */
} smvs_points_options;

typedef struct smvs_points smvs_points;

/* generate_mesh :160-299 with the cut of smvs_cut_depth_maps, on the device,
 * all views at once; options NULL = the reference's defaults (cut, no AABB,
 * dd_factor 5, no faces).  -> a handle holding the points on the host and
 * their number. */
int smvs_points_generate(int device, const smvs_point_view *views, int n_views,
    const smvs_points_options *options, smvs_points **handle,
    int64_t *n_points);
/* Number of points and of triangles (0 unless want_faces; a mesh handle's
 * faces) of a handle. */
int smvs_points_info(const smvs_points *handle, int64_t *n_points,
    int64_t *n_faces);
/* The point attributes (mve::TriangleMesh vertices, vertex normals, colours,
 * confidences and values as save_ply_mesh writes them); any pointer may be
 * NULL.  xyz / normals: n_points*3 floats; rgb: n_points*3 bytes (the image's
 * bytes: ci / 255 stored as uchar); confidence / value: n_points floats;
 * faces: n_faces*3 vertex ids (depthmap_triangulate's face list, merged). */
int smvs_points_download(const smvs_points *handle, float *xyz, float *normals,
    uint8_t *rgb, float *confidence, float *value, uint32_t *faces);
int smvs_points_release(smvs_points *handle);

/* smvsrecon --mesh without --simplify (app/smvsrecon.cc:306-324): per view
 * the triangulation and confidences of smvs_points_generate, merged with
 * mve::geom::mesh_merge in view-list order (mesh_generator.cc:279-282; face
 * ids offset by the vertices before them), optionally clipped with
 * delete_vertices_fix_faces (the faces that lose a corner go, the rest keep
 * their order; vertices no face uses any more are kept), then
 * recalc_normals' angle-weighted vertex normals.  The semantics pinned for
 * the MVE pieces are rows M1-M6 of DESIGN.md section 9.5.  options NULL =
 * the reference's defaults (cut, no AABB, dd_factor 5).  The handle is read
 * with smvs_points_info / smvs_points_download and freed with
 * smvs_points_release; it has no values (a non-NULL value pointer is an
 * argument error) and always the faces. */
typedef struct {
    int cut_surfaces;     /* MeshGenerator::Options::cut_surfaces (--no-cut: 0) */
    int use_aabb;         /* --aabb: delete vertices outside [aabb_min, aabb_max] */
    float aabb_min[3], aabb_max[3];
    float dd_factor;      /* depthmap_triangulate's discontinuity factor, 5 */
} smvs_mesh_options;

int smvs_mesh_generate(int device, const smvs_point_view *views, int n_views,
    const smvs_mesh_options *options, smvs_points **handle,
    int64_t *n_vertices, int64_t *n_faces);

/* Volumetric fusion of the depth maps into ONE surface mesh (not in the
 * reference, opt-in): a truncated signed distance field
 * averaged over all views on a voxel grid, and a surface-nets mesh of its zero
 * level.  This comment is the definition; tests/tsdf_ref.py restates it in
 * numpy and the device agrees with it to the bit.  All arithmetic is float with
 * FMA contraction off, one operation per operation written here; dot3,
 * world_point and the projection are those of the mesh export.
 *
 * Inputs.  views as smvs_mesh_generate takes them (ray-length depth, camera
 * space normals, a colour image of 1 to 4 channels read as step 8 says, a size
 * per view; cut_depth is not written).  The preparation is the mesh export's
 * (z-depth depth_z and, with cut_surfaces and n_views > 1, the cut map cut).  A
 * view's depth at pixel p is D(p) = depth_z[p] where cut[p] != 0, else 0.
 * normals may be NULL only when cut_surfaces == 0.
 *   trunc <= 0      means 3.0f * voxel_size
 *   min_weight <= 0 means 1
 *
 * Field.  Voxel (i, j, k), x fastest in every array, has the centre
 * c[a] = origin[a] + ((float)idx[a] + 0.5f) * voxel_size.  For the views in
 * list order:
 *   1. proj = KR c - t (three dot3, as the cut computes them)
 *   2. skip the view if proj[2] <= 0
 *   3. u = proj[0] / proj[2], v = proj[1] / proj[2]; skip if u < 0 or v < 0
 *   4. xj = (int)u, yj = (int)v; skip if xj >= width or yj >= height
 *   5. skip if D(xj, yj) == 0
 *   6. sdf = D - proj[2]; skip if sdf < -trunc
 *   7. S += fminf(1.0f, sdf / trunc); W += 1 (uint32)
 *   8. if sdf <= trunc: R, G, B (uint32) += the pixel's bytes (1 or 2
 *      channels, grey: all three its byte 0; 3 or 4 channels: bytes 0..2;
 *      the pixel's other bytes are not read), C += 1
 * F = S / (float)W where W >= min_weight, else NaN ("unknown").
 *
 * Vertices (surface nets).  Cell (i, j, k), 0 <= idx[a] <= dims[a] - 2, has
 * the corners c = dx + 2 dy + 4 dz.  It is complete when no corner is NaN; a
 * corner is inside when F < 0.0f; the cell is active when it is complete and
 * its corners are not all on one side.  Edges, in this order: x (0,1) (2,3)
 * (4,5) (6,7), y (0,2) (1,3) (4,6) (5,7), z (0,4) (1,5) (2,6) (3,7).  For each
 * edge (a, b) with exactly one inside end: t = Fa / (Fa - Fb), the crossing is
 * corner a's centre with t * voxel_size added along the edge's axis.
 *   position    per coordinate the sum of the m crossings in edge order,
 *               starting from 0.0f, divided by (float)m
 *   normal      g[0] = the sum over the four x edges in order, starting from
 *               0.0f, of (Fb - Fa), g[1], g[2] likewise over the y and z edges;
 *               len = sqrtf(dot3(g, g)); g / len, or zero when len == 0.  It
 *               points from inside to outside
 *   colour      per channel, with Rs and Cs the sums of R and C over the 8
 *               corners: (2 Rs + Cs) / (2 Cs) in integer division, 0 when Cs == 0
 *   confidence  (float)(sum of W over the 8 corners) / (float)(8 n_views)
 * Vertex ids are the rank of the active cell in the linear cell index.
 *
 * Faces.  For the grid points P in linear order and for each the axes
 * a = 0, 1, 2 in turn: the edge from P to P + e_a, both ends known and exactly
 * one inside.  With (a, b, c) cyclic the edge is shared by the cells at the
 * (b, c) offsets (-1,-1) (0,-1) (0,0) (-1,0) from P: v0 .. v3.  The quad exists
 * only when all four lie in the grid and are complete (they are then active).
 * P inside: triangles (v0, v1, v2) (v0, v2, v3), else (v0, v2, v1)
 * (v0, v3, v2).  Faces are counter-clockwise seen from outside (the side of
 * F >= 0, the cameras' side), so the face normals agree with the vertex
 * normals.  Where the field is unknown the mesh is open.
 *
 * Refused with SMVS_ERR_INVALID before any device call: n_views < 1 (or
 * > 4096), a voxel_size that is not a positive finite number, a dim < 2 or
 * > 1024, a volume of more than 2^27 voxels (28 bytes of device state per
 * voxel: 3.5 GiB), a non-finite origin or trunc, cut_surfaces with a view's
 * normals missing, a missing depth map or image.  No vertex is not an error:
 * the handle then has 0 points and 0 faces.
 *
 * tsdf / weight (either may be NULL): the whole volume, dims[0] * dims[1] *
 * dims[2] values, NaN = unknown.  The handle is a mesh handle (faces always,
 * no values), read with smvs_points_info / smvs_points_download and freed with
 * smvs_points_release. */
typedef struct {
    int cut_surfaces;
    float origin[3];      /* the low corner of voxel (0, 0, 0) */
    float voxel_size;
    int dims[3];
    float trunc;
    int min_weight;
} smvs_tsdf_options;

int smvs_tsdf_fuse(int device, const smvs_point_view *views, int n_views,
    const smvs_tsdf_options *options, float *tsdf, uint32_t *weight,
    smvs_points **handle, int64_t *n_vertices, int64_t *n_faces);

/* smvs_tsdf_fuse on a brick-sparse volume (opt-in): the
 * same mesh, vertex for vertex and face for face to the bit, from a volume that
 * exists only near the surface, so that grids of up to 4096 voxels per side
 * fit.  tests/tsdf_sparse_ref.py restates this comment on top of tests/
 * tsdf_ref.py.
 *
 * Grid, views, preparation, D, steps 1-8, F, vertices and faces are those of
 * smvs_tsdf_fuse.
 *   brick      8 x 8 x 4 voxels.  Brick (bi, bj, bk) holds the voxels
 *              (8 bi .. 8 bi + 7, 8 bj .. 8 bj + 7, 4 bk .. 4 bk + 3) and has
 *              the linear index (bk * by + bj) * bx + bi, with bx =
 *              ceil(dims[0] / 8), by = ceil(dims[1] / 8), bz = ceil(dims[2] / 4).
 *              Bricks at the high faces may be partial.
 *   seed       a voxel whose C of step 8 is > 0 (some view puts it within the
 *              truncation band); a seed brick holds a seed voxel
 *   allocated  a brick that is a seed brick or has one among its up to 26
 *              neighbours in the brick grid
 * In allocated bricks F, W, R, G, B, C are smvs_tsdf_fuse's; elsewhere F is
 * NaN and the sums are 0.  Every inside corner (F < 0) is a seed, and an active
 * cell and the four cells of a quad lie within one voxel of an inside corner,
 * hence in its brick or a neighbour of it: the cells, vertices and faces are
 * exactly the dense ones.
 *   order      vertex ids are the rank of the active cell by (linear brick
 *              index of the cell's corner 0, then the voxel's index inside the
 *              brick, x fastest over 8 x 8 x 4).  Faces follow the grid points
 *              in that same order and for each point the axes 0, 1, 2, with
 *              smvs_tsdf_fuse's rule for the two triangles.
 * The order is the only difference to smvs_tsdf_fuse, whose order is the linear
 * cell index over the whole grid.
 *
 * max_bricks <= 0 means 1 << 20 bricks; the state is 256 * 28 bytes per
 * allocated brick (7 GiB at 1 << 20), which is stats->state_bytes.  More than
 * 1 << 23 is refused (vertex ids are 32 bits).
 *
 * Refused with SMVS_ERR_INVALID before any device call: everything
 * smvs_tsdf_fuse refuses but its size limits, which become: each dim 2 ..
 * 4096, a brick grid of at most 2^28 bricks, and tsdf or weight asked for on a
 * grid of more than 2^27 voxels.  SMVS_ERR_NOMEM, after the seed and dilation
 * passes and before anything is allocated for the volume, when more than
 * max_bricks bricks are allocated: stats and brick_state are filled, the error
 * text names the count needed, there is no handle.
 *
 * brick_state (may be NULL): bx * by * bz bytes, 0 none, 1 allocated, 2 seed.
 * tsdf / weight (either may be NULL): the whole grid as smvs_tsdf_fuse gives
 * it, NaN / 0 where not allocated.  stats may be NULL.  The handle is a mesh
 * handle as smvs_tsdf_fuse's; smvs_tsdf_vertex_cells gives per vertex the
 * cell's linear index in the whole grid, (k * dims[1] + j) * dims[0] + i
 * (n_vertices values), and is SMVS_ERR_INVALID on any other handle. */
typedef struct {
    int64_t max_bricks;
} smvs_tsdf_sparse_options;

typedef struct {
    int64_t bricks, seed_bricks, allocated_bricks, state_bytes;
} smvs_tsdf_sparse_stats;

int smvs_tsdf_fuse_sparse(int device, const smvs_point_view *views, int n_views,
    const smvs_tsdf_options *options, const smvs_tsdf_sparse_options *sparse,
    uint8_t *brick_state, float *tsdf, uint32_t *weight,
    smvs_tsdf_sparse_stats *stats, smvs_points **handle, int64_t *n_vertices,
    int64_t *n_faces);

int smvs_tsdf_vertex_cells(const smvs_points *handle, int64_t *cell);

/* smvs_tsdf_fuse_sparse with a brick cull in front of its seed pass (opt-in
 * through cull != 0).  The cull decides nothing: a
 * brick it drops provably holds no seed voxel, so brick_state, the stats, the
 * volume and the mesh are smvs_tsdf_fuse_sparse's to the bit; only the number
 * of bricks the exact seed test of step 8 runs on changes.  This comment is
 * the definition of the candidates; tests/tsdf_cull_ref.py restates it.  All of
 * it is double arithmetic, one operation per operation written here, no
 * contraction, sums from left to right; only the pyramid is float, and min and
 * max are exact.
 *
 * Pyramid, per view, of D (the prepared and cut z-depth of smvs_tsdf_fuse).
 *   level 0    implicit: texel (x, y) = (lo, hi) = (D, D) where D < 0 or D > 0,
 *              else (D is 0 or NaN: no such pixel passes steps 5-8)
 *              (+inf, -inf).  It is read from D and not stored.
 *   level l+1  ceil(w_l / 2) x ceil(h_l / 2) texels; texel (x, y) is the min of
 *              lo and the max of hi over the level-l texels (2x .. 2x + 1,
 *              2y .. 2y + 1) that exist.  The levels end at 1 x 1: a 1 x 1 map
 *              has level 0 only.
 *
 * Box of brick (bi, bj, bk): per axis a, with i0 the brick's first voxel index
 * and i1 its last clipped to dims[a] - 1, lo[a] = (double)c(i0), hi[a] =
 * (double)c(i1), c the float voxel centre of smvs_tsdf_fuse.  Float rounding
 * is monotone, so every voxel centre of the brick lies in the box.
 *
 * Per view, per row r of KR and t (widened to double):
 *   a = 0, b = 0, mag = |t[r]|; for k = 0, 1, 2: p = KR[r][k] * lo[k],
 *   q = KR[r][k] * hi[k], a = a + min(p, q), b = b + max(p, q),
 *   mag = mag + |KR[r][k]| * max(|lo[k]|, |hi[k]|)
 *   e = 2^-21 * mag + 2^-140
 *   P_lo[r] = (a - t[r]) - e, P_hi[r] = (b - t[r]) + e
 * The float proj[r] of step 1 of every voxel of the brick lies in [P_lo[r],
 * P_hi[r]]: 2^-21 = 8 u bounds the five float roundings of dot3(...) - t and
 * leaves 3 u for the double roundings here; 2^-140 covers three products that
 * underflow.  If any of the six is not finite the view may seed the brick.
 * Else, with zlo = P_lo[2], zhi = P_hi[2]:
 *   zhi <= 0         the view cannot seed the brick (step 2).
 *   zlo <= 0 < zhi   the pixel range is the whole image.
 *   otherwise        per image axis (r = 0 with n = width, r = 1 with n =
 *                    height): ulo = min(P_lo[r] / zlo, P_lo[r] / zhi), uhi =
 *                    max(P_hi[r] / zlo, P_hi[r] / zhi), both clamped to
 *                    [-4, n + 4]; first = floor(ulo) - 1, last = floor(uhi) + 1
 *                    (the pixel of slack covers the float division of step 3);
 *                    last < 0 or first > n - 1: the view cannot seed the
 *                    brick; else first and last are clipped to 0 .. n - 1.
 * The level is the smallest l with (x_last >> l) - (x_first >> l) <= 1 and the
 * same in y; dlo and dhi are the min of lo and the max of hi over the texels
 * (x_first >> l | x_last >> l, y_first >> l | y_last >> l) of that level.
 * dlo > dhi (no valid pixel): the view cannot seed the brick.  Otherwise, with
 * T = (double)trunc * (1 + 2^-22), the view may seed the brick exactly when
 *   dhi >= max(zlo, 0) - T  and  dlo <= zhi + T.
 * A brick is a candidate when some view may seed it.  DESIGN.md section 9.10
 * proves seed brick => candidate, one inequality per step 1-6 and 8.
 *
 * cull == 0: exactly the launches of smvs_tsdf_fuse_sparse (which forwards
 * here); tested_bricks == bricks and brick_candidate is all 1.  cull != 0: the
 * pyramids (at most 8 w h / 3 bytes per view beside the maps), the cull, and
 * the seed pass on the candidates alone; tested_bricks is their number.
 * brick_candidate (may be NULL): bx * by * bz bytes, 1 where the exact seed
 * test ran.  Everything else, the refusals and SMVS_ERR_NOMEM (which leaves
 * stats and both brick arrays filled) are smvs_tsdf_fuse_sparse's. */
typedef struct {
    int64_t max_bricks;
    int cull;
} smvs_tsdf_sparse_opts;

typedef struct {
    int64_t bricks, seed_bricks, allocated_bricks, state_bytes, tested_bricks;
} smvs_tsdf_sparse_opts_stats;

int smvs_tsdf_fuse_sparse_opts(int device, const smvs_point_view *views, int n_views,
    const smvs_tsdf_options *options, const smvs_tsdf_sparse_opts *sparse,
    uint8_t *brick_state, uint8_t *brick_candidate, float *tsdf, uint32_t *weight,
    smvs_tsdf_sparse_opts_stats *stats, smvs_points **handle, int64_t *n_vertices,
    int64_t *n_faces);

/* The preparation, the pyramids and the cull of smvs_tsdf_fuse_sparse_opts
 * alone: brick_candidate (bx * by * bz bytes) and their number (n_candidates
 * may be NULL).  Refuses what smvs_tsdf_fuse_sparse refuses for the views and
 * the grid, before any device call; images are not read and may be NULL. */
int smvs_tsdf_brick_cull(int device, const smvs_point_view *views, int n_views,
    const smvs_tsdf_options *options, uint8_t *brick_candidate, int64_t *n_candidates);

/* One view's pyramid as smvs_tsdf_fuse_sparse_opts builds it (all views are
 * prepared, and cut with cut_surfaces and n_views > 1): the levels >= 1, each
 * row-major, concatenated from level 1 to the 1 x 1 level, lo and hi apart
 * (either may be NULL; both NULL: only the counts, no device call).  n_texels
 * and n_levels (may be NULL): the texels per array and the number of levels
 * >= 1; a 1 x 1 view has none. */
int smvs_tsdf_depth_pyramid(int device, const smvs_point_view *views, int n_views,
    int cut_surfaces, int view, float *lo, float *hi, int64_t *n_texels, int *n_levels);

/* The componentwise minimum and maximum of world_point over the valid
 * (non-zero) pixels of the maps smvs_tsdf_fuse would fuse: the cut maps with
 * cut_surfaces and n_views > 1, else the depth maps (image and channels are not
 * read).  lo[r] > hi[r] (+inf, -inf) means no valid pixel. */
int smvs_tsdf_bounds(int device, const smvs_point_view *views, int n_views,
    int cut_surfaces, float *lo, float *hi);

/* A persistent volume of smvs_tsdf_fuse (opt-in): the
 * sums of its field kept on the device between calls, so that the views are
 * fused batch by batch, a fusion is resumed from a checkpoint, and the surface
 * is extracted any number of times.  This comment is the definition on top of
 * smvs_tsdf_fuse's paragraphs (Inputs, Field, Vertices, Faces), which it does
 * not repeat; tests/tsdf_volume_ref.py restates it on top of tests/tsdf_ref.py.
 *
 * State.  Per voxel S (float), W (uint32) and (R, G, B, C) (4 x uint32), x
 * fastest: 24 bytes per voxel of device memory the volume owns, and the number
 * of views integrated so far.  create: all zero.  trunc <= 0 means 3.0f *
 * voxel_size, fixed at create.
 *
 * Integrate.  The list is prepared as smvs_tsdf_fuse prepares its list (the
 * cut, with cut_surfaces and n_views > 1, acts among the views of THIS list),
 * and steps 1-8 of Field run for its views in list order, starting from the
 * stored S, W, R, G, B, C instead of from zero: S is continued term by term
 * (S = ((S + a) + b) + ..., never S + (a + b + ...)).  The stored count grows
 * by n_views.  After calls with the lists L1, L2, ... the volume therefore
 * holds the sums of smvs_tsdf_fuse's Field over the concatenated list, with
 * each view's D prepared within its own call.  With cut_surfaces == 0, or with
 * one call, that is smvs_tsdf_fuse itself, to the bit, for every split of the
 * list into consecutive batches.  A voxel no view of the list contributes to
 * is neither read nor written.
 *
 * Extract.  F = S / (float)W where W >= min_weight (<= 0 means 1), else NaN;
 * then Vertices and Faces of smvs_tsdf_fuse, n_views in the confidence being
 * the stored count.  tsdf / weight (either may be NULL) and the handle as
 * smvs_tsdf_fuse gives them.  No state changes.  With no view integrated the
 * handle is empty and tsdf all NaN.
 *
 * download / upload are the checkpoint (S and W: one value per voxel, rgbc: 4
 * per voxel; download's pointers may each be NULL, upload needs all three): a
 * state downloaded and uploaded into a volume of the same options continues to
 * the same bits.  reset zeroes the sums and the count.  info gives back the
 * options (trunc as given to create), the count and the device; each pointer
 * may be NULL.
 *
 * Refused with SMVS_ERR_INVALID before any device call: a NULL volume; at
 * create a voxel_size that is not a positive finite number, a dim < 2 or
 * > 1024, more than 2^27 voxels, a non-finite origin or trunc; per integrate
 * what smvs_tsdf_fuse refuses for its views, and a stored count that would
 * pass 2^24 (255 * count must fit uint32, 8 * count an int); upload with
 * n_views < 0 or > 2^24.  A refused or failed call leaves the state as it was
 * (a failed upload: undefined sums, reset or upload again).  A failed
 * allocation at create is SMVS_ERR_NOMEM and leaves no handle.  Calls on one
 * volume are not to overlap; different volumes are independent. */
typedef struct {
    float origin[3];      /* the low corner of voxel (0, 0, 0) */
    float voxel_size;
    int dims[3];
    float trunc;
} smvs_tsdf_volume_options;
typedef struct smvs_tsdf_volume smvs_tsdf_volume;

int smvs_tsdf_volume_create(int device, const smvs_tsdf_volume_options *options,
    smvs_tsdf_volume **volume);
int smvs_tsdf_volume_integrate(smvs_tsdf_volume *volume, const smvs_point_view *views,
    int n_views, int cut_surfaces);
int smvs_tsdf_volume_extract(const smvs_tsdf_volume *volume, int min_weight, float *tsdf,
    uint32_t *weight, smvs_points **handle, int64_t *n_vertices, int64_t *n_faces);
int smvs_tsdf_volume_info(const smvs_tsdf_volume *volume, smvs_tsdf_volume_options *options,
    int64_t *n_views, int *device);
int smvs_tsdf_volume_download(const smvs_tsdf_volume *volume, float *S, uint32_t *W,
    uint32_t *rgbc);
int smvs_tsdf_volume_upload(smvs_tsdf_volume *volume, const float *S, const uint32_t *W,
    const uint32_t *rgbc, int64_t n_views);
int smvs_tsdf_volume_reset(smvs_tsdf_volume *volume);
void smvs_tsdf_volume_release(smvs_tsdf_volume *volume);

/* A persistent volume of smvs_tsdf_fuse_sparse (opt-in; DESIGN.md section
 * 9.14): the brick-sparse sums kept on the device between calls, so that a
 * grid of up to 4096 voxels per side is fused batch by batch, checkpointed and
 * extracted any number of times.  This comment is the definition on top of the
 * comments of smvs_tsdf_fuse (Inputs, Field, Vertices, Faces),
 * smvs_tsdf_fuse_sparse (brick, seed, the dilation called "allocated" there,
 * the order) and smvs_tsdf_volume_create (continuing the sums), which it does
 * not repeat; tests/tsdf_sparse_volume_ref.py restates it on top of their
 * restatements.
 *
 * Which bricks exist depends on all views, and a brick that gets its storage
 * after some views have passed has missed their free-space terms.  So the
 * table is a state of its own, fixed by mark, and growth reports what it cost.
 *
 * State, owned on the device.  One seed byte per brick of the grid; the table
 * brick -> slot and the list slot -> brick, the slots always in linear brick
 * order over the bricks that have storage; per slot birth, the stored view
 * count at the start of the integrate that gave the brick its slot; per voxel
 * of a slot, slot-major (slot * 256 + the voxel's index in the brick), S
 * (float), W (uint32) and (R, G, B, C) (4 x uint32): 24 bytes per voxel, 6144
 * per slot; and the number of views integrated so far.  F and the vertex ids
 * are not state.  create: no seed, no slot, count 0.  trunc <= 0 means 3.0f *
 * voxel_size, fixed at create.  max_bricks <= 0 means 1 << 20.
 *
 * mark(list, cut_surfaces, cull).  The list is prepared as
 * smvs_tsdf_fuse_sparse prepares its list, and the seed bytes are OR-ed with
 * that entry's seed rule on this list: a brick is a seed when it holds a voxel
 * where some view of the list passes steps 1-6 with sdf <= trunc.  With cull
 * the cull of smvs_tsdf_fuse_sparse_opts runs in front and decides nothing.
 * No sum is touched and no slot is given; images are not read and may be NULL.
 * The dilation (every seed brick and its up to 26 neighbours) of the would-be
 * seed set is counted before the OR is committed: more than max_bricks is
 * SMVS_ERR_NOMEM, the error text names the count needed, nothing changes.
 *
 * integrate(list, cut_surfaces, grow, cull).  The list is prepared once.  With
 * grow != 0 the list is marked first, under the same budget rule, checked
 * before anything is committed.  Then every brick of the dilation of the seeds
 * that has no slot gets one: the table is rebuilt in linear brick order, the
 * sums move to their new slots, new bricks start at zero with birth = the
 * stored count.  Then steps 1-8 of Field run for the list's views in list
 * order on every brick that has a slot, continuing the stored sums term by
 * term as smvs_tsdf_volume_integrate does: a voxel no view of the list
 * contributes to is neither read nor written.  The count grows by n_views.
 *
 * So a brick holds Field's sums over the views of index >= its birth, in list
 * order from zero.  If every mark precedes the first integrate (all birth = 0)
 * the state on the bricks with slots is the dense persistent volume's state
 * there, and with cut_surfaces == 0, or with one batch, the extracted mesh,
 * cells, brick_state, tsdf and weight are smvs_tsdf_fuse_sparse's over the
 * concatenated list, to the bit, for every split into consecutive batches.
 * With the cut on, the cut acts within a batch, as for smvs_tsdf_volume.  A
 * brick with birth > 0 is LATE: stats.late_bricks == 0 is how a caller learns
 * that the identity holds.
 *
 * Slots that the one-shot would not have (marks of views that are never
 * integrated) do not change the mesh: an inside corner (F < 0) needs a view
 * with -trunc <= sdf < 0 there, which makes its brick a seed of the integrated
 * views; and every cell that holds a seed voxel lies within the seed brick and
 * its 26 neighbours.  Outside the one-shot's bricks F is >= 0 or NaN, and the
 * cells, vertices and faces are the one-shot's.
 *
 * extract(min_weight).  F = S / (float)W where W >= min_weight (<= 0 means 1),
 * else NaN, on the bricks with slots, NaN elsewhere; then Vertices and Faces
 * of smvs_tsdf_fuse_sparse in (slot, index in brick) order, n_views in the
 * confidence being the stored count.  The handle (smvs_tsdf_vertex_cells
 * answers it), tsdf and weight (either may be NULL; only for grids of at most
 * 2^27 voxels) as smvs_tsdf_fuse_sparse gives them; brick_state (may be NULL):
 * 0 / 1 / 2 from the seeds as marked.  Extract changes no state, and marks not
 * yet followed by an integrate do not affect the mesh, tsdf or weight.
 *
 * info.  stats: bricks of the grid, seed bricks, allocated_bricks (with
 * slots), pending_bricks (in the dilation, without a slot), late_bricks,
 * state_bytes (6144 per slot) and the view count.  Each pointer may be NULL.
 *
 * download / upload are the checkpoint: brick_state (bricks bytes), list and
 * birth (allocated_bricks values each), S and W (256 per slot), rgbc (1024 per
 * slot) and the count.  download's pointers may each be NULL.  upload checks
 * before any device call: brick_state holds 0, 1, 2 (only 2 is read: the
 * seeds); n_slots is 0 .. max_bricks, n_views 0 .. 2^24, the seeds' dilation
 * has at most max_bricks bricks; the list is strictly ascending, inside the
 * grid and inside the dilation of the uploaded seeds; no birth is above
 * n_views.  A state uploaded into a fresh volume of the same options continues
 * to the same bits.  reset: no seed, no slot, count 0.
 *
 * Refused with SMVS_ERR_INVALID before any device call: a NULL volume; at
 * create what smvs_tsdf_fuse_sparse refuses for its grid (a dim < 2 or > 4096,
 * more than 2^28 bricks, max_bricks > 2^23, voxel_size, origin, trunc); per
 * mark and integrate what smvs_tsdf_fuse refuses for its views (mark needs no
 * image), and a stored count that would pass 2^24; at extract tsdf or weight
 * on a grid of more than 2^27 voxels.  A refused or failed call leaves the
 * state as it was (a failed upload: undefined, reset or upload again).  During
 * a re-slot the old and the new sums exist side by side: 6144 bytes times (old
 * + new slots) at the peak.  Calls on one volume are not to overlap; different
 * volumes are independent. */
typedef struct {
    float origin[3];      /* the low corner of voxel (0, 0, 0) */
    float voxel_size;
    int dims[3];
    float trunc;
    int64_t max_bricks;
} smvs_tsdf_sparse_volume_options;

typedef struct {
    int64_t bricks, seed_bricks, allocated_bricks, pending_bricks, late_bricks, state_bytes,
        n_views;
} smvs_tsdf_sparse_volume_stats;

typedef struct smvs_tsdf_sparse_volume smvs_tsdf_sparse_volume;

int smvs_tsdf_sparse_volume_create(int device, const smvs_tsdf_sparse_volume_options *options,
    smvs_tsdf_sparse_volume **volume);
int smvs_tsdf_sparse_volume_mark(smvs_tsdf_sparse_volume *volume, const smvs_point_view *views,
    int n_views, int cut_surfaces, int cull);
int smvs_tsdf_sparse_volume_integrate(smvs_tsdf_sparse_volume *volume,
    const smvs_point_view *views, int n_views, int cut_surfaces, int grow, int cull);
int smvs_tsdf_sparse_volume_extract(const smvs_tsdf_sparse_volume *volume, int min_weight,
    uint8_t *brick_state, float *tsdf, uint32_t *weight, smvs_points **handle,
    int64_t *n_vertices, int64_t *n_faces);
int smvs_tsdf_sparse_volume_info(const smvs_tsdf_sparse_volume *volume,
    smvs_tsdf_sparse_volume_options *options, smvs_tsdf_sparse_volume_stats *stats, int *device);
int smvs_tsdf_sparse_volume_download(const smvs_tsdf_sparse_volume *volume, uint8_t *brick_state,
    uint32_t *list, uint32_t *birth, float *S, uint32_t *W, uint32_t *rgbc);
int smvs_tsdf_sparse_volume_upload(smvs_tsdf_sparse_volume *volume, const uint8_t *brick_state,
    const uint32_t *list, const uint32_t *birth, int64_t n_slots, const float *S,
    const uint32_t *W, const uint32_t *rgbc, int64_t n_views);
int smvs_tsdf_sparse_volume_reset(smvs_tsdf_sparse_volume *volume);
void smvs_tsdf_sparse_volume_release(smvs_tsdf_sparse_volume *volume);

/* Cleaning a triangle mesh (not in the reference, whose documented pipeline
 * ends with MVE's `meshclean -p10`; opt-in): a cut on
 * the vertex confidences, then the removal of small connected components and
 * of vertices no face uses.  MVE is not part of this project: the definition
 * is this comment, tests/mesh_clean_ref.py restates it in numpy, and the device
 * agrees with it to the bit.  Everything below is a fact of the input -- a
 * partition, integer counts, an order statistic -- so nothing is rounded.
 *
 * Input.  n vertices with xyz, normals (3 floats each), rgb (3 bytes),
 * confidence (1 float) and optionally cells (int64, the sparse fusion's cell
 * per vertex); m faces of three uint32 vertex ids.
 *
 * 1. Cut value t.
 *      percentile == 0   t = threshold; threshold <= 0 means no cut
 *      0 < percentile <= 100
 *                        k = (int64)((double)percentile * (double)(n - 1) /
 *                        100.0); t is the k-th smallest confidence, 0-based,
 *                        in the order of the key u ^ (u >> 31 ? 0xFFFFFFFF :
 *                        0x80000000) on the float's bits u (-0.0 sorts below
 *                        0.0, a NaN by its sign beyond the infinities).
 *                        n == 0 means no cut
 *    Both non-zero is SMVS_ERR_INVALID.  Vertex v is cut when confidence[v] <
 *    t, a float comparison: a NaN confidence is never cut, a NaN t cuts
 *    nothing.  "No cut" is t = -inf.
 * 2. Faces, first pass.  A face survives when none of its corners is cut and
 *    its three ids are pairwise different.
 * 3. Components.  Two uncut vertices are linked when a surviving face holds
 *    both; components are the transitive closure.  A component's size is its
 *    number of vertices; an uncut vertex in no surviving face is a component
 *    of size 1.  A vertex is small when its component has fewer than
 *    component_size vertices; component_size <= 1 makes nothing small.
 * 4. Unreferenced.  Unless keep_unreferenced != 0, an uncut vertex in no
 *    surviving face is dropped whatever component_size is.
 * 5. Result.  The vertices that are not cut, not small and not dropped, in
 *    input order; new id = rank.  Every attribute (and cells) is copied bit for
 *    bit; normals are not recomputed.  The surviving faces whose corners all
 *    remain, in input order, ids renumbered.  An empty result is not an error.
 *
 * Optional outputs per INPUT vertex (each may be NULL):
 *   component       uint32: the smallest vertex id of the vertex's component,
 *                   0xFFFFFFFF for a cut vertex
 *   component_size  uint32: the component's size, 0 for a cut vertex
 *   new_id          int64: the vertex's id in the result, -1 when it is removed
 * stats (may be NULL): cut_value = t; n_cut the cut vertices; n_components the
 * components of step 3 (those of size 1 included); n_small_components and
 * n_small_vertices the components below component_size and their vertices;
 * n_unreferenced the uncut vertices in no surviving face (kept or not);
 * largest_component the largest size, 0 without a component.
 *
 * Refused with SMVS_ERR_INVALID before any device call: n or m negative or
 * above 2^31 - 1; a face id >= n (one host pass over the faces); a percentile
 * outside [0, 100] or not finite; a threshold that is not finite; threshold and
 * percentile both non-zero; a missing array with n > 0 (faces with m > 0).
 *
 * The handle is a mesh handle (smvs_points_info / _download / _release; no
 * values).  It answers smvs_tsdf_vertex_cells exactly when cells was given.
 * smvs_mesh_clean_handle cleans the mesh a handle holds (cells when it is a
 * sparse fusion's) and is SMVS_ERR_INVALID on a handle without faces: a point
 * cloud's that kept none.  (A mesh handle with 0 faces has faces.)  A point
 * cloud's values are not carried over. */
typedef struct {
    float threshold;        /* meshclean -t; 0: off */
    float percentile;       /* meshclean -p; 0: off */
    int component_size;     /* meshclean -c */
    int keep_unreferenced;
} smvs_mesh_clean_options;

typedef struct {
    float cut_value;
    int64_t n_cut, n_components, n_small_components, n_small_vertices, n_unreferenced,
        largest_component;
} smvs_mesh_clean_stats;

int smvs_mesh_clean(int device, int64_t n, int64_t m, const float *xyz, const float *normals,
    const uint8_t *rgb, const float *confidence, const int64_t *cells, const uint32_t *faces,
    const smvs_mesh_clean_options *options, uint32_t *component, uint32_t *component_size,
    int64_t *new_id, smvs_mesh_clean_stats *stats, smvs_points **handle, int64_t *n_vertices,
    int64_t *n_faces);

int smvs_mesh_clean_handle(int device, const smvs_points *in,
    const smvs_mesh_clean_options *options, uint32_t *component, uint32_t *component_size,
    int64_t *new_id, smvs_mesh_clean_stats *stats, smvs_points **handle, int64_t *n_vertices,
    int64_t *n_faces);

/* smvsrecon --simplify (MeshGenerator::Options::simplify, mesh_generator.cc:
 * 238-243): per view DepthTriangulator::approximate_triangulation
 * (depth_triangulator.cc:27-172) -- Garland and Heckbert's greedy insertion
 * into an incremental Delaunay triangulation (delaunay_2d.cc, quad_edge.h) --
 * instead of the full triangulation, then the confidences, scale values,
 * normal lookup and merge of smvs_points_generate / smvs_mesh_generate on the
 * irregular meshes.  Rows S1-S13 of DESIGN.md section 9.7 pin the semantics.
 * One persistent workgroup per view runs the insertion loop.
 *   create_triangle_mesh  0: the point cloud (values, looked-up normals; the
 *                            faces too unless use_aabb), 1: the mesh of
 *                            --mesh --simplify (recalc_normals, no values)
 *   max_vertices          -1: pixels / 40; the number of loop ITERATIONS (S1)
 *   max_error             -1.0: (max depth - mean depth) * 1e-3 (S2)
 * options NULL = the reference's defaults (cut, no AABB, point cloud, -1, -1).
 * Refused as argument errors: image size != depth size is the caller's to
 * keep (one width / height per view), width or height < 2 or > 4096,
 * non-finite or negative depths.  A view whose loop hits a safety cap (the
 * walks over the subdivision are bounded) ends the call with SMVS_ERR_STATE. */
typedef struct {
    int cut_surfaces;     /* MeshGenerator::Options::cut_surfaces (--no-cut: 0) */
    int use_aabb;         /* --aabb: delete vertices outside [aabb_min, aabb_max] */
    float aabb_min[3], aabb_max[3];
    int create_triangle_mesh;
    int max_vertices;
    double max_error;
} smvs_simplify_options;

int smvs_simplified_generate(int device, const smvs_point_view *views, int n_views,
    const smvs_simplify_options *options, smvs_points **handle,
    int64_t *n_vertices, int64_t *n_faces);

/* The greedy triangulation of ONE depth map in pixel space, before any
 * clean-up (S1-S8), so that a divergence from the restatement can be located
 * at the insertion where it happens.  Outputs (any may be NULL):
 *   iterations       loop iterations run (S1: no-op insertions count)
 *   vertices         n_vertices * 3 doubles (x, y, z), the four corners first;
 *                    room for min(budget, pixels) + 5 vertices
 *   triangles        n_triangles * 3 vertex ids per triangle id (S4's order);
 *                    room for twice as many triangles as vertices
 *   num_zero_depths  per triangle
 *   clocks4          100 MHz ticks the workgroup spent in selection, the
 *                    Delaunay lane, the rescans, and in total */
int smvs_simplify_triangulate(int device, const float *depth, int width, int height,
    int max_vertices, double max_error, int64_t *iterations, int64_t *n_vertices,
    double *vertices, int64_t *n_triangles, uint32_t *triangles,
    int32_t *num_zero_depths, uint64_t *clocks4);

/* smvsrecon's input scaling (app/smvsrecon.cc:634-647): `halvings` chained
 * mve::image::rescale_half_size_gaussian<uint8_t> (sigma^2 = 0.75,
 * [MVE-unverified] M29) of one interleaved u8 image on the device, bit-identical
 * with the host mirror's function (host/scene_io.cc); the intermediate levels
 * stay on the device.  out receives the last level, ((w + 1) / 2 per halving) x
 * ((h + 1) / 2 ...) x channels bytes, *out_width / *out_height its size.
 * Argument errors (SMVS_ERR_INVALID, before any device call): a null pointer,
 * halvings < 1, channels outside 1..4, a level whose input is narrower or lower
 * than 2 pixels ("image too small", as the host function), out_capacity below
 * the last level's bytes. */
int smvs_rescale_half_gaussian(int device, const uint8_t *pixels, int width, int height,
    int channels, int halvings, uint8_t *out, size_t out_capacity, int *out_width,
    int *out_height);

/* Undistortion: one interleaved u8 image of a camera with lens distortion, an
 * off-centre principal point or non-square pixels, resampled on the device
 * into the pinhole camera the rest of this library works with -- focal length
 * out_focal pixels, principal point (out_width / 2, out_height / 2), square
 * pixels (CameraInfo carries only flen).  The importer of COLMAP models
 * (host/colmap_io.h) calls it per image; it has no counterpart in the
 * reference.
 *
 * One form of the lens covers COLMAP's SIMPLE_PINHOLE (f, cx, cy), PINHOLE
 * (fx, fy, cx, cy), SIMPLE_RADIAL (f, cx, cy, k), RADIAL (f, cx, cy, k1, k2)
 * and OPENCV (fx, fy, cx, cy, k1, k2, p1, p2); parameters a model lacks are
 * zero and their terms then vanish exactly.
 *
 * Per output pixel (x, y), everything in float, one rounding per operation,
 * no contraction, in this order; inv = (float)(1.0 / (double)out_focal) is
 * formed on the host:
 *   u  = (((float)x + 0.5f) - 0.5f*(float)out_width ) * inv
 *   v  = (((float)y + 0.5f) - 0.5f*(float)out_height) * inv
 *   uu = u*u;  vv = v*v;  r2 = uu + vv;  uv = u*v
 *   rad = 1.0f + r2*(k1 + k2*r2)
 *   du = (2.0f*p1)*uv + p2*(r2 + 2.0f*uu)
 *   dv = p1*(r2 + 2.0f*vv) + (2.0f*p2)*uv
 *   sx = ((fx*(u*rad + du)) + cx) - 0.5f
 *   sy = ((fy*(v*rad + dv)) + cy) - 0.5f
 * The pixel is inside iff 0 <= sx <= width - 1 and 0 <= sy <= height - 1 (a NaN
 * is outside).  Inside, each channel is Image<uint8_t>::linear_at
 * ([MVE-unverified] M3): x0 = (int)sx, x1 = min(x0 + 1, width - 1), the same in
 * y; w1 = sx - x0, w0 = 1 - w1, w3 = sy - y0, w2 = 1 - w3;
 * v00*w0*w2 + v10*w1*w2 + v01*w0*w3 + v11*w1*w3 with the products and the sum
 * left to right, then + 0.5f and truncated.  Outside, every channel is 0 and
 * the pixel counts in *blank_pixels (may be NULL).  For a source f that is a
 * power of two, a centred principal point and out_focal = f, out equals pixels
 * byte for byte.
 *
 * Argument errors (SMVS_ERR_INVALID, before any device call; out untouched):
 * a null pixels, lens or out, channels outside 1..4, any size below 1,
 * out_focal not positive (or not finite), a non-finite lens value, an image of
 * more than 2^31 bytes. */
typedef struct {
    float fx, fy, cx, cy, k1, k2, p1, p2;   /* source camera, pixels; COLMAP convention:
                                               the centre of pixel (0,0) is (0.5,0.5) */
} smvs_lens;
int smvs_undistort_u8(int device, const uint8_t *pixels, int width, int height, int channels,
    const smvs_lens *lens, float out_focal, int out_width, int out_height,
    uint8_t *out, int64_t *blank_pixels /* may be NULL */);

/* The context-free entry points above (smvs_sgm_run, smvs_sgm_depth_for_view,
 * smvs_bilateral_upsample, smvs_cut_depth_maps) draw their device buffers,
 * stream and pinned staging memory from a per-device pool of workspaces that
 * is kept between calls (the reference allocates its volumes per SGMStereo
 * object, lib/sgm_stereo.cc:192-225; a device allocation per call costs more
 * than the kernels).  Concurrent callers get different workspaces.  This
 * returns the pooled memory (workspaces and parked contexts) to the driver;
 * -> number of objects freed. */
int smvs_release_workspaces(void);

/* ------------------------------------------------------------------ */
/* measurement                                                        */
/* ------------------------------------------------------------------ */

/* Kernel classes timed with HIP events on the context's stream. */
enum {
    SMVS_K_PATCH = 0,     /* per-patch J^T W J + g  (K1-K4) */
    SMVS_K_ASSEMBLE,      /* block gather + 4x4 LDL (K5)    */
    SMVS_K_CG_SPMV,       /* block-stencil SpMV + d.Ad (K6) */
    SMVS_K_CG_UPDATE,     /* x, r, z update + reductions (K7/K8) */
    SMVS_K_CG_INIT,
    SMVS_K_REACTIVATE,    /* K9 */
    SMVS_K_MISC,
    SMVS_K_CG_RESIDENT,   /* whole PCG solve in one launch, H in registers */
    SMVS_K_COUNT
};
/* Kernel classes of the context-free front end (SGM, bilateral upsample),
 * timed with HIP events on the call's workspace stream while enabled.
 * smvs_sgm_profile returns the accumulated ms / launches (either may be NULL)
 * and then, if enable >= 0, switches the timing on (1) or off (0) and clears
 * the accumulators; enable < 0 only reads. */
enum {
    SMVS_SGM_K_CENSUS = 0,   /* census of the main image (K11) */
    SMVS_SGM_K_WARP,         /* plane-sweep warp (K12) */
    SMVS_SGM_K_COST,         /* census of the warped planes + Hamming cost (K11, K13) */
    SMVS_SGM_K_PATHS,        /* 8-path aggregation (K14) */
    SMVS_SGM_K_WTA,          /* argmin + depth (K15) */
    SMVS_SGM_K_LR_CHECK,     /* left / right consistency (K16); in the plane sweep the one
                              * support kernel (it has no left / right check) */
    SMVS_SGM_K_MERGE,        /* two-neighbour merge (K16); with SMVS_SGM_MERGE_CONSENSUS the one
                              * check-and-merge kernel (then no SMVS_SGM_K_LR_CHECK launches);
                              * in the plane sweep the one fold of the n cost volumes */
    SMVS_SGM_K_BILATERAL,    /* joint bilateral upsample (K17) */
    SMVS_SGM_K_COUNT
};
int smvs_sgm_profile(int enable, double *ms, long long *launches);

int smvs_profile_enable(smvs_ctx *ctx, int on);
int smvs_profile_reset(smvs_ctx *ctx);
/* ms[SMVS_K_COUNT] accumulated kernel time, launches[SMVS_K_COUNT] */
int smvs_profile_get(smvs_ctx *ctx, double *ms, long long *launches);

#ifdef __cplusplus
}
#endif
#endif /* SMVS_HIP_H */
