// What the translation units of the SGM front end share: sgm.hip (run_sgm:
// census, warp, cost), sgm_paths.hip (its path aggregation), sgm_wta.hip (its
// winner-takes-all), sgm_view.hip (a view's front end), sgm_sweep.hip (the
// opt-in plane sweep over n neighbours), sgm_speckle.hip (the opt-in speckle
// removal), sgm_photo.hip (the opt-in multi-view photo-consistency test),
// sgm_refine.hip (the opt-in multi-view plane refinement sweeps), image_prep.hip
// (a view's input image), bilateral.hip (the joint bilateral upsample).
#pragma once

#include "common.h"
#include "sgm_path_plan.h"

#include <vector>

namespace smvs_hip {

// Optional per-kernel timing of the front end (smvs_sgm_profile): HIP events
// on the workspace's stream around every launch of a call, read back when the
// call has synchronised.  Off by default: no events, no overhead.  (The
// counters and the two members that touch them: sgm.hip.)
struct SgmProfile {
    struct Pending { int cls; hipEvent_t a, b; };
    std::vector<Pending> pending;
    bool on;
    SgmProfile();
    // (called when the stream is idle)
    ~SgmProfile();
};

struct SgmKernelTimer {
    SgmProfile *prof;
    hipStream_t stream;
    int cls;
    hipEvent_t a = nullptr, b = nullptr;
    SgmKernelTimer(SgmProfile *p, hipStream_t s, int c) : prof(p), stream(s), cls(c)
    {
        if (prof == nullptr || !prof->on)
            return;
        (void)hipEventCreate(&a);
        (void)hipEventCreate(&b);
        (void)hipEventRecord(a, stream);
    }
    ~SgmKernelTimer()
    {
        if (a == nullptr)
            return;
        (void)hipEventRecord(b, stream);
        prof->pending.push_back({ cls, a, b });
    }
};

// Slots of a pooled workspace (pool.hip) used by the front end.
enum {
    WS_DEPTHS = 0, WS_CENSUS, WS_WARPED, WS_COST, WS_SGM, WS_ARGMIN,   // one run_sgm
    WS_MAIN, WS_NBR0, WS_NBR1, WS_FWD0, WS_FWD1, WS_BWD, WS_COST16,   // a view's front end
    WS_RAW, WS_RAW0, WS_RAW1,                                         // raw u8 images + scratch
    WS_BIL_DM, WS_BIL_CI, WS_BIL_OUT,                                 // bilateral upsample
    WS_DELTA,                                                         // eight path-byte volumes
    WS_FWDN, WS_BWDN, WS_SUPPORT,                                     // consensus merge: n + n maps, support
    WS_SWEEP,                                                         // plane sweep: n cost volumes
    WS_SPECKLE, WS_RUNNER_UP,                                         // filters: labels + counts, runner-up map
    WS_PHOTO, WS_PHOTO_OUT,                                           // photo test: witness images; confidence + views
    WS_REFINE                                                         // refinement: a, gx, gy; the slants
};
static_assert(WS_REFINE < Workspace::SLOTS, "the last slot must exist in a Workspace");

// The largest plane count of a run: the key of the WTA kernels is
// value * 256 + plane (one byte for the plane), and 64 lanes x 4 planes is one
// wavefront per line in sgm_paths_wide_kernel.
constexpr int SGM_MAX_PLANES = 256;

// The plane counts a run takes: 2 .. 128 (any), and the multiples of 8 from 136
// to SGM_MAX_PLANES.  Why 8: SGMStereo::Options::num_steps is a free integer,
// but the reference's default build (SMVS_ENABLE_SSE) aggregates in groups of
// eight planes (lib/sgm_stereo.cc:355-356, 377, 399, 416) and is only defined
// for multiples of eight; the counts up to 128 keep what they always took.
__host__ __device__ __forceinline__ constexpr bool
sgm_plane_count_ok(int num_steps)
{
    return (num_steps >= 2 && num_steps <= 128)
        || (num_steps > 128 && num_steps <= SGM_MAX_PLANES && (num_steps % 8) == 0);
}
static_assert(sgm_plane_count_ok(2) && sgm_plane_count_ok(127) && sgm_plane_count_ok(136)
        && sgm_plane_count_ok(256) && !sgm_plane_count_ok(1) && !sgm_plane_count_ok(129)
        && !sgm_plane_count_ok(132) && !sgm_plane_count_ok(264), "the plane-count rule");

// Work buffers of one run_sgm inside a pooled workspace; reused by the runs of
// a view (the runs are ordered on the workspace's stream).  Every run has its
// own depth table: SGM_MAX_PLANES depths, then as many inverse depths (the
// sub-plane winner's).  The uniqueness test of a call (include/smvs_hip.h,
// "uniqueness test") is the workspace's, since every run of a view makes it:
// uniqueness == 0 launches the WTA kernels without it.  MAX_RUNS: two runs per
// neighbour of the consensus front end (64 KB of tables).
struct SgmWorkspace {
    static constexpr int MAX_RUNS = 2 * SMVS_MAX_SUBS;
    Workspace *ws;
    SgmProfile *prof = nullptr;
    float *depths = nullptr;
    unsigned long long *census = nullptr;
    uint8_t *warped = nullptr, *cost = nullptr;
    uint16_t *sgm = nullptr;     // S: only when the caller wants it or the DELTA form does not apply
    uint8_t *delta = nullptr;    // the eight path-byte volumes of the DELTA form
    int32_t *argmin = nullptr;
    int runs = 0;
    bool want_sgm = false;       // smvs_sgm_run hands the S volume to its caller
    int uniqueness = 0, uniqueness_window = 1;
    uint16_t *runner_up = nullptr;   // optional output of the uniqueness WTA kernels
    explicit SgmWorkspace(Workspace *w) : ws(w) {}
    // the uniqueness test of a *_filtered entry's options; null: off
    void set_filter(const smvs_sgm_filter_options *filter)
    {
        uniqueness = filter != nullptr ? filter->uniqueness : 0;
        uniqueness_window = filter != nullptr ? filter->uniqueness_window : 1;
    }
    // the largest penalty2 a step can use: the option itself, or in the adaptive
    // mode max(P2 / diff, P1 * 3 / 2) <= max(P2, P1 * 3 / 2)
    static unsigned largest_penalty2(unsigned penalty1, unsigned penalty2, int p2_mode)
    {
        unsigned const floor_value = penalty1 * 3u / 2u;
        return p2_mode == SMVS_SGM_P2_ADAPTIVE && floor_value > penalty2 ? floor_value
                                                                        : penalty2;
    }
    int ensure(size_t npix, int num_steps, SgmPathPlan const &plan)
    {
        size_t const vol = npix * (size_t)num_steps;
        int rc;
        if ((rc = ws->ensure(WS_DEPTHS, (size_t)2 * SGM_MAX_PLANES * MAX_RUNS, &depths))
            || (rc = ws->ensure(WS_CENSUS, npix, &census))
            || (rc = ws->ensure(WS_WARPED, vol, &warped))
            || (rc = ws->ensure(WS_COST, vol, &cost))
            || (rc = ws->ensure(WS_ARGMIN, npix, &argmin)))
            return rc;
        if (plan.delta && (rc = ws->ensure(WS_DELTA, 8 * vol, &delta)))
            return rc;
        if (plan.needs_s(want_sgm) && (rc = ws->ensure(WS_SGM, vol, &sgm)))
            return rc;
        return SMVS_OK;
    }
};

// The small checks, none of which involves a device; check_sgm_view_call and
// the entries outside it (the runs, smvs_sgm_check_merge, smvs_sgm_fold_costs,
// smvs_sgm_filter_speckles) are made of them.
// p2_mode and the penalties:
int check_sgm_penalties(unsigned penalty1, unsigned penalty2, int p2_mode);
// sgm_plane_count_ok:
int check_sgm_plane_count(int num_steps);
// smvs_sgm_options: non-NULL, a known winner
int check_sgm_winner(const smvs_sgm_options *opts);
// smvs_sgm_view_options and the neighbour count: non-NULL, a known winner and
// merge, one or two neighbours for the reference's merge; for the consensus
// 1 .. SMVS_MAX_SUBS neighbours, agree_ratio in [0, 1] (a NaN is none) and
// min_agree in 1 .. SMVS_MAX_SUBS.  (sgm_view.hip)
int check_sgm_view_options(const smvs_sgm_view_options *opts, int n_neighbors);
// smvs_sgm_filter_options: non-NULL, uniqueness in 0 .. 99, the window in
// 1 .. 256, speckle_size >= 0, speckle_ratio in [0, 1] (a NaN is none);
// run_entry: the speckle fields must be off.  (sgm.hip)
int check_sgm_filter(const smvs_sgm_filter_options *filter, bool run_entry);
// Whether the speckle filter of the options runs at all (sizes 0 and 1 remove
// nothing).
inline bool
sgm_speckle_on(const smvs_sgm_filter_options *filter)
{
    return filter != nullptr && filter->speckle_size > 1;
}
// speckle_size and speckle_ratio alone.  (sgm_speckle.hip)
int check_sgm_speckle(int speckle_size, float speckle_ratio);
// The two words per pixel the speckle kernels work in (slot WS_SPECKLE).
int sgm_speckle_ensure(Workspace &ws, size_t npix, uint32_t **d_words);
// Speckle removal of d_depth[w * h] into d_out (may be d_depth) on the
// workspace's stream, four launches under timers of class SMVS_SGM_K_MERGE (three
// for a map of one tile); want_size: the component sizes are left in
// d_words[0 .. w * h).  hipGetLastError.  (sgm_speckle.hip)
int sgm_launch_speckle(Workspace &ws, SgmProfile *prof, const float *d_depth, int w, int h,
    int speckle_size, float speckle_ratio, uint32_t *d_words, float *d_out, bool want_size);

// The photo-consistency test of include/smvs_hip.h ("Multi-view
// photo-consistency test"): radius 0 is off.
inline bool
sgm_photo_on(const smvs_sgm_photo_options *photo)
{
    return photo != nullptr && photo->radius > 0;
}
// smvs_sgm_photo_options for n witnesses in all: radius in 0 .. 3, best_k and
// min_views in 0 .. n, min_score in [-1, 1] (a NaN is none).  (sgm_photo.hip)
int check_sgm_photo(const smvs_sgm_photo_options *photo, int n);
// One witness of the test on the device: its SGM-scale image and the float
// reprojection main -> witness.
struct SgmPhotoWitness {
    const uint8_t *image;
    int nw, nh;
    float M[9], t[3];
};
// The test of d_depth[w * h] against n witnesses (1 .. SMVS_MAX_SUBS) into d_out
// (may be d_depth), d_confidence and d_views (either may be null) on the
// workspace's stream: one launch under a timer of class SMVS_SGM_K_MERGE.
// hipGetLastError.  (sgm_photo.hip)
int sgm_launch_photo(Workspace &ws, SgmProfile *prof, const uint8_t *d_main, int w, int h,
    const float *d_depth, const SgmPhotoWitness *witnesses, int n,
    smvs_sgm_photo_options const &opts, float *d_out, float *d_confidence, uint8_t *d_views);

// The plane refinement sweeps of include/smvs_hip.h ("Multi-view plane
// refinement sweeps"): sweeps 0 is off.
inline bool
sgm_refine_on(const smvs_sgm_refine_options *refine)
{
    return refine != nullptr && refine->sweeps > 0;
}
// smvs_sgm_refine_options: non-NULL, sweeps and samples in 0 .. 8, depth_step and
// slant_step in [0, 1] (a NaN is none), fill 0 or 1.  (sgm_refine.hip)
int check_sgm_refine(const smvs_sgm_refine_options *refine);
// Floats per pixel of slot WS_REFINE: the state planes a, gx, gy, then the slant
// output [h][w][2].  (The state's confidence and views are the photo test's
// outputs, slot WS_PHOTO_OUT.)
constexpr size_t SGM_REFINE_PLANES = 5;
// The refinement of d_depth[w * h] against n witnesses into d_out (may be
// d_depth), d_slant (may be null), d_confidence and d_views (the state: neither
// may be null) on the workspace's stream, with d_state[3 * w * h] to work in: a
// start launch, 2 * sweeps half-sweep launches, an end launch, each under a timer
// of class SMVS_SGM_K_MERGE.  hipGetLastError.  (sgm_refine.hip)
int sgm_launch_refine(Workspace &ws, SgmProfile *prof, const uint8_t *d_main, int w, int h,
    const float *d_depth, const SgmPhotoWitness *witnesses, int n,
    smvs_sgm_photo_options const &photo, smvs_sgm_refine_options const &refine, float *d_state,
    float *d_out, float *d_slant, float *d_confidence, uint8_t *d_views);

// What a run is asked for besides its images and depth range: the options of
// SGMStereo (num_steps, the penalties), smvs_sgm_p2_mode and smvs_sgm_winner.
// Each entry fills one and every stage of the run reads it.
struct SgmRunParams {
    int num_steps;
    uint16_t penalty1, penalty2;
    int p2_mode, winner;
};

// The plan of a run (sgm_path_plan.h) with this process's SMVS_SGM_PATHS: `wave`
// asks for a wave per line, two planes per lane, up to 128 planes.
// (sgm_paths.hip)
SgmPathPlan sgm_path_plan_here(int num_steps, unsigned largest_p2);

// aggregate_sgm_costs (sgm_stereo.cc:429-667) on B.cost: what lies between the
// cost kernels and the WTA kernels of a run -- S zeroed where the plan asks
// for it, the launches of the plan's form under a timer of class
// SMVS_SGM_K_PATHS, hipGetLastError.  The path bytes go to B.delta or the sums
// to B.sgm, as plan.delta says.  (sgm_paths.hip)
int sgm_launch_paths(SgmWorkspace &B, SgmPathPlan const &plan, const uint8_t *d_main,
    int w, int h, SgmRunParams const &P);

// The stages of a run, which sgm_run_device and the plane sweep of
// sgm_sweep.hip share.  (sgm.hip)
struct SgmRun {
    SgmPathPlan plan;
    const float *d_depths = nullptr, *d_inv = nullptr;   // this run's tables in B.depths
    bool subplane = false;
};
// The checks of a run, its plan, B's buffers for w x h x num_steps and the run's
// depth table (sgm_stereo.cc:195-203) uploaded.
int sgm_run_plan(SgmWorkspace &B, int w, int h, float min_depth, float max_depth,
    SgmRunParams const &P, SgmRun *R);
// census_filter of the main image into B.census
void sgm_launch_census(SgmWorkspace &B, const uint8_t *d_main, int w, int h);
// warped_neighbors_for_depth and create_cost_volume for one neighbour: through
// B.warped into d_cost (B.cost, or a volume of the sweep); hipGetLastError
int sgm_launch_warp_cost(SgmWorkspace &B, SgmRun const &R, int w, int h,
    const uint8_t *d_nbr, int nw, int nh, const float *M, const float *t, int num_steps,
    uint8_t *d_cost);
// depth_from_sgm_volume (sgm_stereo.cc:274-306) behind sgm_launch_paths: the
// WTA kernel of (R.plan.wta, R.subplane, B.uniqueness != 0) under a timer of
// class SMVS_SGM_K_WTA, hipGetLastError.  d_depth, B.argmin (B.sgm with
// B.want_sgm, B.runner_up where set).  (sgm_wta.hip)
int sgm_launch_wta(SgmWorkspace &B, SgmRun const &R, const uint8_t *d_main, size_t npix,
    int num_steps, float *d_depth);
// sgm_launch_paths on B.cost, then sgm_launch_wta
int sgm_run_tail(SgmWorkspace &B, SgmRun const &R, const uint8_t *d_main, int w, int h,
    SgmRunParams const &P, float *d_depth);
// a u8 cost volume on the device, widened to u16, to the host (slot WS_COST16)
int sgm_download_cost16(Workspace &ws, const uint8_t *d_cost, size_t vol, uint16_t *cost);

// SGMStereo::run_sgm (sgm_stereo.cc:98-124) on device images; the depth map
// (and optionally argmin) stay on the device.  Asynchronous on the workspace's
// stream.  (sgm.hip)
int sgm_run_device(SgmWorkspace &B, const uint8_t *d_main, int w, int h, const uint8_t *d_nbr,
    int nw, int nh, const float *M, const float *t, float min_depth, float max_depth,
    SgmRunParams const &P, float *d_depth);

// One view's SGM input image on the device: upload (raw: interleaved u8 of
// `channels`; otherwise already at SGM scale, one channel), desaturate and
// `halvings` half-size steps.  *out (slot `slot_out`) receives the image,
// *ow / *oh its size.  (image_prep.hip)
int sgm_prepare_image(Workspace &ws, const uint8_t *host, int w, int h, int channels,
    int halvings, int slot_out, int slot_tmp, uint8_t **out, int *ow, int *oh);
// What sgm_prepare_image makes of w x h x channels in `halvings` steps: the
// SGM-scale size ((s + 1) >> 1 per halving) and the bytes it asks of its two
// slots (tmp 0: the slot is not touched).  A front that sends several images
// through one pair of slots sizes them with this.  (image_prep.hip)
struct SgmPreparedSize {
    int w, h;
    size_t out, tmp;
};
SgmPreparedSize sgm_prepared_size(int w, int h, int channels, int halvings);

// ------------------------------------------------- a view entry's call record
// What one of the 18 smvs_sgm_depth_for_view* / smvs_sgm_sweep_for_view*
// entries is asked for (include/smvs_hip.h: which entry fixes which field).
// The entries at SGM scale are the raw ones with channels = 1, SGM_ONE_CHANNEL
// and halvings = 0; the entries without filters those with SGM_FILTERS_OFF; the
// 14 without the photo test those with SGM_PHOTO_OFF and no further witness; the
// 16 without the refinement those with SGM_REFINE_OFF and no slant.
// neighbors and neighbor_channels hold n_neighbors + n_witness entries: the
// first n_neighbors go through the front, all of them are witnesses of the test.
struct SgmViewCall {
    int device;
    const uint8_t *main_img;
    int w, h, channels;
    const smvs_sgm_neighbor *neighbors;
    const int *neighbor_channels;
    int n_neighbors, halvings;
    SgmRunParams P;
    bool sweep;                     // the front: the sweep, or that of view_opts.merge
    smvs_sgm_view_options view_opts;    // (p2_mode and winner of both: as in P)
    smvs_sgm_sweep_options sweep_opts;
    const float *range;             // the sweep's depth range
    const smvs_sgm_filter_options *filter;
    const char *null_options;       // the entry's options pointer was null: the refusal
    float *depth, *checked;         // outputs; null: not asked for
    uint8_t *support;
    int32_t *argmin;
    uint16_t *cost, *sgm, *runner_up;
    int n_witness;                  // the photo test: entries of `neighbors` behind n_neighbors
    const smvs_sgm_photo_options *photo;
    float *confidence;              // its outputs; null: not asked for
    uint8_t *views;
    const smvs_sgm_refine_options *refine;  // the refinement sweeps, in the photo test's place
    float *slant;                   // their output [h][w][2]; null: not asked for
};
constexpr int SGM_ONE_CHANNEL[SMVS_MAX_SUBS] = { 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1 };
static_assert(SMVS_MAX_SUBS == 16, "SGM_ONE_CHANNEL: one entry per neighbour");
// (what SgmWorkspace::set_filter and sgm_speckle_on make of it: nothing runs)
constexpr smvs_sgm_filter_options SGM_FILTERS_OFF = { 0, 1, 0, 0.95f };
// (what sgm_photo_on makes of it: no launch; best_k and min_views pass the check
// for every neighbour count)
constexpr smvs_sgm_photo_options SGM_PHOTO_OFF = { 0, 0, 0, 0.49f };
// (what sgm_refine_on makes of it: the photo test's launch, or none)
constexpr smvs_sgm_refine_options SGM_REFINE_OFF = { 0, 2, 0.02f, 0.01f, 1u, 1 };

// Every refusal of a view entry, before its first device call, in the one
// order written above it.  (sgm_view.hip)
int check_sgm_view_call(SgmViewCall const &C);
// smvs_sgm_sweep_options and the neighbour count, as the checks above.  (sgm_sweep.hip)
int check_sgm_sweep_options(const smvs_sgm_sweep_options *opts, int n_neighbors);

// What the three fronts share of one call: the leased workspace, the timers,
// the run buffers, the main image at SGM scale, the speckle words, the
// witnesses of the photo test.  (sgm_view.hip)
struct SgmViewSession {
    SgmViewCall const &C;
    WorkspaceLease lease;
    SgmProfile prof;                // (destroyed before the lease: the stream is idle then)
    SgmWorkspace B;
    uint8_t *d_main = nullptr;
    int mw = 0, mh = 0;
    size_t npix = 0;
    uint32_t *d_speckle = nullptr;
    // the photo test: every witness image at SGM scale in one slot (WS_PHOTO),
    // confidence and views behind each other in another (WS_PHOTO_OUT)
    SgmPhotoWitness witness[SMVS_MAX_SUBS];
    uint8_t *d_witness = nullptr, *d_views = nullptr;
    size_t witness_at[SMVS_MAX_SUBS + 1] = { 0 };
    float *d_confidence = nullptr;
    float *d_refine = nullptr;      // the refinement's planes (WS_REFINE), when it is on
    explicit SgmViewSession(SgmViewCall const &call) : C(call), lease(call.device), B(lease.w) {}
    Workspace &ws() { return *lease.w; }
    // the call's filter and want_sgm, the main image prepared (WS_MAIN, WS_RAW),
    // the speckle words when the filter asks; with the photo test its two slots
    // and the witnesses behind the front's neighbours, prepared and kept
    int open();
    // neighbour k prepared into the two slots (and kept as witness k of the
    // photo test)
    int neighbor(int k, int slot_out, int slot_tmp, uint8_t **d_nbr, int *nw, int *nh);
    // B's buffers for runs on images of up to largest_pix pixels
    int ensure_runs(size_t largest_pix);
    // SGMStereo::reconstruct, sgm_stereo.cc:46-62: main -> neighbour k, then
    // neighbour k -> main with the neighbour's own depth range
    int run_pair(int k, const uint8_t *d_nbr, int nw, int nh, float *d_fwd, float *d_bwd);
    // the photo test on d_map when on (with the refinement sweeps on: those in its
    // place), the speckle filter on d_map when on, then the outputs the call asks
    // for
    int finish(float *d_map, const float *d_checked, const uint8_t *d_support);
};
// check, session, front: what every view entry does with its record
int sgm_run_view_call(SgmViewCall const &C);
// the sweep front of an open session (sgm_sweep.hip)
int sgm_front_sweep(SgmViewSession &S, SgmViewCall const &C);

// The eight path directions (dx, dy) in the reference's order: ->, <-, then
// the three top-to-bottom paths, then the three bottom-to-top paths.  The host
// launches in this order, the all-direction kernels decode blockIdx.x in it.
constexpr int SGM_DIRS[8][2] = { { 1, 0 }, { -1, 0 }, { 0, 1 }, { 1, 1 }, { -1, 1 },
    { 0, -1 }, { 1, -1 }, { -1, -1 } };

// Lines of direction k in a w x h image: the rows of a horizontal path, the
// columns of a vertical one, every diagonal that starts on the entry row or
// the entry column of a diagonal one.
__host__ __device__ __forceinline__ constexpr int
sgm_dir_lines(int k, int w, int h)
{
    return SGM_DIRS[k][1] == 0 ? h : (SGM_DIRS[k][0] == 0 ? w : w + h - 1);
}

// Grid of the all-direction kernels: a block per line (sgm_all_paths_kernel,
// sgm_paths_wide_kernel), or per pair of adjacent lines of one direction (sgm_paths2_kernel).  The
// kernels find (direction, line) by walking the same counts.
__host__ __device__ __forceinline__ constexpr int
sgm_grid_lines(int w, int h)
{
    int n = 0;
    for (int k = 0; k < 8; ++k)
        n += sgm_dir_lines(k, w, h);
    return n;
}
__host__ __device__ __forceinline__ constexpr int
sgm_grid_line_pairs(int w, int h)
{
    int n = 0;
    for (int k = 0; k < 8; ++k)
        n += (sgm_dir_lines(k, w, h) + 1) / 2;
    return n;
}
// the sums written out; odd and even w and h at the smallest image
// smvs_sgm_run accepts, and an ordinary one
constexpr bool
sgm_grids_agree(int w, int h)
{
    int const d = w + h - 1;
    return sgm_grid_lines(w, h) == h + h + w + d + d + w + d + d
        && sgm_grid_line_pairs(w, h) == 2 * ((h + 1) / 2 + (w + 1) / 2) + 4 * ((d + 1) / 2);
}
static_assert(sgm_grids_agree(11, 9) && sgm_grids_agree(12, 9) && sgm_grids_agree(11, 10)
        && sgm_grids_agree(64, 48), "grid size and per-direction line counts disagree");
// (sgm_all_paths_kernel finds the two horizontal directions by one division)
static_assert(sgm_dir_lines(0, 64, 48) == sgm_dir_lines(1, 64, 48), "directions 0, 1: rows");

} // namespace smvs_hip
