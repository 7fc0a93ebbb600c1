// A view's SGM front end on gfx950: SGMStereo::reconstruct (reference:
// lib/sgm_stereo.cc:46-91) -- run_sgm main -> neighbour and back (sgm.hip), the
// left/right consistency check -- and the two-neighbour merge of
// reconstruct_sgm_depth_for_view (app/smvsrecon.cc:360-377), on images that
// image_prep.hip brought to SGM scale; and, opt-in, the same front end over up
// to SMVS_MAX_SUBS neighbours with the checks and an n-neighbour consensus in
// one kernel (SMVS_SGM_MERGE_CONSENSUS).
#include "sgm_internal.h"

namespace smvs_hip {

// ------------------------------------------------------- L/R check + merge
// SGMStereo::reconstruct, sgm_stereo.cc:64-91: the main view's depth is kept
// where its correspondence in the neighbour (integer pixel coordinates, no
// +0.5; Correspondence in double from the float M, t) lies inside the 3 %
// border and the neighbour's own depth agrees within a factor 0.8; truncating
// lookup.  Operation order of correspondence.cc:20-51, contraction off.
struct LrArgs {
    float *d_main;
    const float *d_neig;
    int w, h, nw, nh, cut;
    double M[9], t[3];
};

__global__ void __launch_bounds__(256)
sgm_lr_check_kernel(LrArgs A)
{
#pragma clang fp contract(off)
    int const x = blockIdx.x * blockDim.x + threadIdx.x;
    int const y = blockIdx.y;
    if (x >= A.w)
        return;
    size_t const o = (size_t)y * A.w + x;
    float const dm = A.d_main[o];
    if (dm == 0.0f)
        return;
    double const u = (double)x, v = (double)y, wd = (double)dm;
    double const p = A.M[0] * u + A.M[1] * v + A.M[2];
    double const q = A.M[3] * u + A.M[4] * v + A.M[5];
    double const r = A.M[6] * u + A.M[7] * v + A.M[8];
    double const a = wd * p + A.t[0];
    double const b = wd * q + A.t[1];
    double const d = wd * r + A.t[2];
    double const cx = a / d, cy = b / d;
    if (cx < (double)A.cut || cx >= (double)(A.nw - A.cut)
        || cy < (double)A.cut || cy >= (double)(A.nh - A.cut)) {
        A.d_main[o] = 0.0f;
        return;
    }
    float const cdepth = (float)d;
    float const ndepth = A.d_neig[(size_t)(int)cy * A.nw + (size_t)(int)cx];
    float const ratio = fminf(cdepth, ndepth) / fmaxf(cdepth, ndepth);
    if (ndepth == 0.0f || (double)ratio < 0.8)
        A.d_main[o] = 0.0f;
}

// app/smvsrecon.cc:366-377: average where both maps are valid
__global__ void __launch_bounds__(256)
sgm_merge_kernel(float *__restrict__ d1, const float *__restrict__ d2, size_t n)
{
#pragma clang fp contract(off)
    size_t const i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    float const b = d2[i];
    if (b == 0.0f)
        return;
    float const a = d1[i];
    d1[i] = a == 0.0f ? b : (a + b) * 0.5f;
}

// ------------------------------------------- n checks + consensus, one kernel
// SMVS_SGM_MERGE_CONSENSUS (include/smvs_hip.h has the definition): per pixel
// the n left/right checks above -- each neighbour with its own reprojection in
// double, its own nw / nh / cut and its own truncating lookup -- and the
// consensus over the n checked depths.  The forward maps are read once; the
// merged map, and the checked maps and the support when asked for, are written
// once.  `checked` may be `fwd` itself (a thread reads and writes its own pixel).
struct CheckNeighbor {
    const float *bwd;
    int nw, nh, cut, pad;
    double M[9], t[3];
};
struct CheckMergeArgs {
    const float *fwd;       // [n][h][w]
    float *merged;          // [h][w] or null
    float *checked;         // [n][h][w] or null
    uint8_t *support;       // [h][w] or null
    int w, h, min_agree;
    float agree_ratio;
    CheckNeighbor nb[SMVS_MAX_SUBS];
};
static_assert(sizeof(CheckMergeArgs) <= 4096, "kernel arguments: 4 KB at the most");

// sgm_lr_check_kernel's test of one depth against one neighbour: the depth, or 0.
// (One difference where that kernel is undefined: a correspondence that is not a
// number, from a projective depth of 0, fails the border test here -- the
// comparisons are written so that a NaN is outside -- where there it would go
// on to an undefined lookup.)
__device__ __forceinline__ float
lr_checked_depth(float dm, int x, int y, CheckNeighbor const &N)
{
#pragma clang fp contract(off)
    if (dm == 0.0f)
        return 0.0f;
    double const u = (double)x, v = (double)y, wd = (double)dm;
    double const p = N.M[0] * u + N.M[1] * v + N.M[2];
    double const q = N.M[3] * u + N.M[4] * v + N.M[5];
    double const r = N.M[6] * u + N.M[7] * v + N.M[8];
    double const a = wd * p + N.t[0];
    double const b = wd * q + N.t[1];
    double const d = wd * r + N.t[2];
    double const cx = a / d, cy = b / d;
    if (!(cx >= (double)N.cut && cx < (double)(N.nw - N.cut)
            && cy >= (double)N.cut && cy < (double)(N.nh - N.cut)))
        return 0.0f;
    float const cdepth = (float)d;
    float const ndepth = N.bwd[(size_t)(int)cy * N.nw + (size_t)(int)cx];
    float const ratio = fminf(cdepth, ndepth) / fmaxf(cdepth, ndepth);
    if (ndepth == 0.0f || (double)ratio < 0.8)
        return 0.0f;
    return dm;
}

// N is a template parameter so that every loop over the neighbours unrolls and
// c[] and star[] are registers (an array indexed by a run-time value would go
// to scratch; the code object's .private_segment_fixed_size is 0 for all 16).
// star[k]: bit j set when c[j] supports c[k]; the ratio of a pair is symmetric
// (fminf / fmaxf of the same two numbers), so each pair is divided once.
template <int N>
__global__ void __launch_bounds__(256)
sgm_check_merge_kernel(CheckMergeArgs A)
{
#pragma clang fp contract(off)
    size_t const npix = (size_t)A.w * A.h;
    size_t const o = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= npix)
        return;
    int const y = (int)(o / (size_t)A.w);
    int const x = (int)(o - (size_t)y * A.w);
    float c[N];
    unsigned star[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        c[k] = lr_checked_depth(A.fwd[(size_t)k * npix + o], x, y, A.nb[k]);
        star[k] = c[k] != 0.0f ? 1u << k : 0u;
    }
    if (A.checked != nullptr) {
#pragma unroll
        for (int k = 0; k < N; ++k)
            A.checked[(size_t)k * npix + o] = c[k];
    }
#pragma unroll
    for (int k = 0; k < N; ++k) {
#pragma unroll
        for (int j = k + 1; j < N; ++j) {
            bool const agree = c[k] != 0.0f && c[j] != 0.0f
                && fminf(c[j], c[k]) / fmaxf(c[j], c[k]) >= A.agree_ratio;
            star[k] |= agree ? 1u << j : 0u;
            star[j] |= agree ? 1u << k : 0u;
        }
    }
    int best_count = 0;
    unsigned best_star = 0u;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        int const count = __popc(star[k]);
        bool const better = count > best_count;     // strict: ties keep the lowest k
        best_star = better ? star[k] : best_star;
        best_count = better ? count : best_count;
    }
    float out = 0.0f;
    if (best_count != 0 && best_count >= A.min_agree) {
        float s = 0.0f;
#pragma unroll
        for (int j = 0; j < N; ++j)
            s = (best_star >> j) & 1u ? s + c[j] : s;
        out = s / (float)best_count;
    }
    if (A.merged != nullptr)
        A.merged[o] = out;
    if (A.support != nullptr)
        A.support[o] = (uint8_t)best_count;
}

template <int N>
static void
launch_check_merge_n(CheckMergeArgs const &A, int n, unsigned blocks, hipStream_t stream)
{
    if constexpr (N > SMVS_MAX_SUBS)
        return;
    else if (n == N)
        hipLaunchKernelGGL(sgm_check_merge_kernel<N>, dim3(blocks), dim3(256), 0, stream, A);
    else
        launch_check_merge_n<N + 1>(A, n, blocks, stream);
}

// the fused kernel for n neighbours, under a timer of class SMVS_SGM_K_MERGE
static int
launch_check_merge(CheckMergeArgs const &A, int n, SgmProfile *prof, hipStream_t stream)
{
    size_t const npix = (size_t)A.w * A.h;
    {
        SgmKernelTimer timer(prof, stream, SMVS_SGM_K_MERGE);
        launch_check_merge_n<1>(A, n, (unsigned)((npix + 255) / 256), stream);
    }
    SMVS_HIP_CHECK(hipGetLastError());
    return SMVS_OK;
}

// The 3 % border of the left/right check in a neighbour of nw x nh
// (sgm_stereo.cc:70-71), and the float reprojection of an entry widened to the
// doubles both check kernels compute in.
static int
lr_cut(int nw, int nh)
{
    return (int)(0.03 * (double)(nw > nh ? nw : nh));
}

static void
widen_reprojection(double *M, double *t, const float *M_fwd, const float *t_fwd)
{
    for (int i = 0; i < 9; ++i)
        M[i] = (double)M_fwd[i];
    for (int i = 0; i < 3; ++i)
        t[i] = (double)t_fwd[i];
}

static LrArgs
fill_lr_args(float *d_fwd, const float *d_bwd, int w, int h, int nw, int nh, const float *M_fwd,
    const float *t_fwd)
{
    LrArgs L = { d_fwd, d_bwd, w, h, nw, nh, lr_cut(nw, nh), {}, {} };
    widen_reprojection(L.M, L.t, M_fwd, t_fwd);
    return L;
}

static void
fill_check_neighbor(CheckNeighbor *C, const float *d_bwd, int nw, int nh, const float *M_fwd,
    const float *t_fwd)
{
    *C = { d_bwd, nw, nh, lr_cut(nw, nh), 0, {}, {} };
    widen_reprojection(C->M, C->t, M_fwd, t_fwd);
}

// The fused kernel's arguments behind nb[0 .. n), which the caller has filled:
// the unused neighbours are copies of nb[0], the checked maps go where the
// forward maps are (a thread reads and writes its own pixel).
static void
fill_check_merge(CheckMergeArgs *A, int n, float *d_fwd, float *d_merged, bool want_checked,
    uint8_t *d_support, int w, int h, int min_agree, float agree_ratio)
{
    for (int k = n; k < SMVS_MAX_SUBS; ++k)
        A->nb[k] = A->nb[0];
    A->fwd = d_fwd;
    A->merged = d_merged;
    A->checked = want_checked ? d_fwd : nullptr;
    A->support = d_support;
    A->w = w;
    A->h = h;
    A->min_agree = min_agree;
    A->agree_ratio = agree_ratio;
}

// (declared in sgm_internal.h)
int
check_sgm_view_options(const smvs_sgm_view_options *opts, int n_neighbors)
{
    SMVS_REQUIRE(opts != nullptr, "null options (p2_mode, winner, merge)");
    SMVS_REQUIRE(opts->winner == SMVS_SGM_WINNER_PLANE
            || opts->winner == SMVS_SGM_WINNER_SUBPLANE, "unknown winner");
    SMVS_REQUIRE(opts->merge == SMVS_SGM_MERGE_REFERENCE
            || opts->merge == SMVS_SGM_MERGE_CONSENSUS, "unknown merge");
    if (opts->merge == SMVS_SGM_MERGE_REFERENCE) {
        SMVS_REQUIRE(n_neighbors >= 1 && n_neighbors <= 2,
            "one or two neighbours (app/smvsrecon.cc:360-365)");
        return SMVS_OK;
    }
    SMVS_REQUIRE(n_neighbors >= 1 && n_neighbors <= SMVS_MAX_SUBS,
        "n_neighbors must be in [1, SMVS_MAX_SUBS]");
    // (a NaN fails both comparisons)
    SMVS_REQUIRE(opts->agree_ratio >= 0.0f && opts->agree_ratio <= 1.0f,
        "agree_ratio must be in [0, 1]");
    SMVS_REQUIRE(opts->min_agree >= 1 && opts->min_agree <= SMVS_MAX_SUBS,
        "min_agree must be in [1, SMVS_MAX_SUBS]");
    return SMVS_OK;
}

// (declared in sgm_internal.h)  The one order of the checks, for all 18 entries.
// No check involves a device, and a later one may rely on an earlier one (the
// neighbour arrays are read once the count is known to fit them).
//   1. the entry's options pointer            2. the filter options
//   3. p2_mode, winner, merge
//   4. the neighbour count: 1 .. 2 for the reference's merge, 1 .. SMVS_MAX_SUBS
//      for the consensus and the sweep
//   5. the front's options: agree_ratio, min_agree; min_views, best_k,
//      support_cost, min_support
//   6. the plane count                        7. the penalties, in both modes
//   8. the sweep's depth range
//   9. null pointers: the images, depth (optional in the sweep), neighbor_channels
//  10. the channels of the main image, then of each neighbour
//  11. halvings
//  12. the main image's size at SGM scale, then each neighbour's: above 10 x 8
//      where the neighbour gets a run of its own, above 1 x 1 in the sweep
//  13. outputs the options exclude: checked and support with the reference's
//      merge, runner_up without the uniqueness test
//  14. the photo test: the options pointer; radius, best_k, min_views, min_score;
//      the witness count; with radius 0 no witness, confidence or views; each
//      witness behind the front's neighbours: its image, size and channels
//  15. the refinement sweeps: the options pointer; sweeps, samples; depth_step,
//      slant_step; fill; sweeps > 0 with photo radius 0; a slant output with
//      sweeps 0
int
check_sgm_view_call(SgmViewCall const &C)
{
    int rc;
    SMVS_REQUIRE(C.null_options == nullptr, C.null_options);
    if ((rc = check_sgm_filter(C.filter, false)) != SMVS_OK)
        return rc;
    SMVS_REQUIRE(C.P.p2_mode == SMVS_SGM_P2_CONSTANT || C.P.p2_mode == SMVS_SGM_P2_ADAPTIVE,
        "unknown penalty2 mode");
    rc = C.sweep ? check_sgm_sweep_options(&C.sweep_opts, C.n_neighbors)
                 : check_sgm_view_options(&C.view_opts, C.n_neighbors);
    if (rc != SMVS_OK || (rc = check_sgm_plane_count(C.P.num_steps)) != SMVS_OK
        || (rc = check_sgm_penalties(C.P.penalty1, C.P.penalty2, C.P.p2_mode)) != SMVS_OK)
        return rc;
    if (C.sweep) {
        SMVS_REQUIRE(C.range != nullptr, "null argument (range)");
        // (a NaN fails the comparisons)
        SMVS_REQUIRE(C.range[0] > 0.f && C.range[1] > C.range[0],
            "bad depth range: 0 < min_depth < max_depth");
    }
    SMVS_REQUIRE(C.main_img && C.neighbors && (C.sweep || C.depth) && C.neighbor_channels,
        "null argument");
    SMVS_REQUIRE(C.channels == 1 || C.channels == 3, "1 or 3 channels");
    for (int k = 0; k < C.n_neighbors; ++k)
        SMVS_REQUIRE(C.neighbor_channels[k] == 1 || C.neighbor_channels[k] == 3,
            "1 or 3 channels");
    SMVS_REQUIRE(C.halvings >= 0 && C.halvings <= 8, "halvings out of range");
    SMVS_REQUIRE((C.w >> C.halvings) > 10 && (C.h >> C.halvings) > 8, "image too small");
    int const least_w = C.sweep ? 1 : 10, least_h = C.sweep ? 1 : 8;
    for (int k = 0; k < C.n_neighbors; ++k)
        SMVS_REQUIRE(C.neighbors[k].image && (C.neighbors[k].width >> C.halvings) > least_w
                && (C.neighbors[k].height >> C.halvings) > least_h, "bad neighbour image");
    if (!C.sweep && C.view_opts.merge == SMVS_SGM_MERGE_REFERENCE)
        SMVS_REQUIRE(C.checked == nullptr && C.support == nullptr,
            "checked and support are outputs of the consensus merge");
    SMVS_REQUIRE(C.runner_up == nullptr || C.filter->uniqueness != 0,
        "runner_up is an output of the uniqueness test (uniqueness > 0)");
    int const n_all = C.n_neighbors + C.n_witness;
    if ((rc = check_sgm_photo(C.photo, n_all)) != SMVS_OK)
        return rc;
    SMVS_REQUIRE(C.n_witness >= 0 && n_all <= SMVS_MAX_SUBS,
        "n_witness must not be negative, n_neighbors + n_witness at most SMVS_MAX_SUBS");
    if (!sgm_photo_on(C.photo))
        SMVS_REQUIRE(C.n_witness == 0 && C.confidence == nullptr && C.views == nullptr,
            "witnesses, confidence and views belong to the photo test (photo radius > 0)");
    for (int k = C.n_neighbors; k < n_all; ++k) {
        SMVS_REQUIRE(C.neighbors[k].image && (C.neighbors[k].width >> C.halvings) >= 1
                && (C.neighbors[k].height >> C.halvings) >= 1, "bad witness image");
        SMVS_REQUIRE(C.neighbor_channels[k] == 1 || C.neighbor_channels[k] == 3,
            "1 or 3 channels (witness)");
    }
    if ((rc = check_sgm_refine(C.refine)) != SMVS_OK)
        return rc;
    SMVS_REQUIRE(!sgm_refine_on(C.refine) || sgm_photo_on(C.photo),
        "refine sweeps > 0 need the photo test's window and witnesses (photo radius > 0)");
    SMVS_REQUIRE(C.slant == nullptr || sgm_refine_on(C.refine),
        "slant is an output of the refinement sweeps (refine sweeps > 0)");
    return SMVS_OK;
}

// ------------------------------------------------------------ the session
int
SgmViewSession::open()
{
    if (lease.w == nullptr)
        return SMVS_ERR_HIP;
    B.prof = &prof;
    B.want_sgm = C.sgm != nullptr;
    B.set_filter(C.filter);
    int rc;
    if ((rc = sgm_prepare_image(ws(), C.main_img, C.w, C.h, C.channels, C.halvings, WS_MAIN,
             WS_RAW, &d_main, &mw, &mh)) != SMVS_OK)
        return rc;
    npix = (size_t)mw * mh;
    if (sgm_speckle_on(C.filter) && (rc = sgm_speckle_ensure(ws(), npix, &d_speckle)) != SMVS_OK)
        return rc;
    if (!sgm_photo_on(C.photo))
        return SMVS_OK;
    // the photo test's slots at their final size, then the witnesses the front
    // does not prepare, through the slots of neighbour 0: all before the
    // front's first SGM launch
    int const n_all = C.n_neighbors + C.n_witness;
    for (int k = 0; k < n_all; ++k) {
        SgmPreparedSize const Z = sgm_prepared_size(C.neighbors[k].width, C.neighbors[k].height,
            C.neighbor_channels[k], C.halvings);
        witness_at[k + 1] = witness_at[k] + (((size_t)Z.w * Z.h + 15) & ~(size_t)15);
    }
    if ((rc = ws().ensure(WS_PHOTO, witness_at[n_all], &d_witness))
        || (rc = ws().ensure(WS_PHOTO_OUT, npix * (sizeof(float) + 1), &d_confidence)))
        return rc;
    d_views = reinterpret_cast<uint8_t *>(d_confidence + npix);
    if (sgm_refine_on(C.refine)
        && (rc = ws().ensure(WS_REFINE, npix * SGM_REFINE_PLANES, &d_refine)))
        return rc;
    for (int k = C.n_neighbors; k < n_all; ++k) {
        uint8_t *d_img = nullptr;
        int pw = 0, ph = 0;
        if ((rc = neighbor(k, WS_NBR0, WS_RAW0, &d_img, &pw, &ph)) != SMVS_OK)
            return rc;
    }
    return SMVS_OK;
}

int
SgmViewSession::neighbor(int k, int slot_out, int slot_tmp, uint8_t **d_nbr, int *nw, int *nh)
{
    smvs_sgm_neighbor const &N = C.neighbors[k];
    int const rc = sgm_prepare_image(ws(), N.image, N.width, N.height, C.neighbor_channels[k],
        C.halvings, slot_out, slot_tmp, d_nbr, nw, nh);
    if (rc != SMVS_OK || !sgm_photo_on(C.photo))
        return rc;
    // kept for the photo test (the slot may hold the next neighbour by then)
    SgmPhotoWitness &W = witness[k];
    uint8_t *const kept = d_witness + witness_at[k];
    SMVS_HIP_CHECK(hipMemcpyAsync(kept, *d_nbr, (size_t)*nw * *nh, hipMemcpyDeviceToDevice,
        ws().stream));
    W.image = kept;
    W.nw = *nw;
    W.nh = *nh;
    for (int i = 0; i < 9; ++i)
        W.M[i] = N.M_fwd[i];
    for (int i = 0; i < 3; ++i)
        W.t[i] = N.t_fwd[i];
    return SMVS_OK;
}

int
SgmViewSession::ensure_runs(size_t largest_pix)
{
    return B.ensure(largest_pix, C.P.num_steps, sgm_path_plan_here(C.P.num_steps,
        SgmWorkspace::largest_penalty2(C.P.penalty1, C.P.penalty2, C.P.p2_mode)));
}

int
SgmViewSession::run_pair(int k, const uint8_t *d_nbr, int nw, int nh, float *d_fwd, float *d_bwd)
{
    smvs_sgm_neighbor const &N = C.neighbors[k];
    int const rc = sgm_run_device(B, d_main, mw, mh, d_nbr, nw, nh, N.M_fwd, N.t_fwd,
        N.range_main[0], N.range_main[1], C.P, d_fwd);
    return rc != SMVS_OK ? rc : sgm_run_device(B, d_nbr, nw, nh, d_main, mw, mh, N.M_bwd,
        N.t_bwd, N.range_neighbor[0], N.range_neighbor[1], C.P, d_bwd);
}

int
SgmViewSession::finish(float *d_map, const float *d_checked, const uint8_t *d_support)
{
    int rc;
    Workspace &w = ws();
    // (behind the merge or the support test, the photo test first: the components
    // are those of the map that leaves; checked and support are those of the
    // unfiltered map)
    bool const photo = sgm_photo_on(C.photo), refine = sgm_refine_on(C.refine);
    float *const d_slant = refine ? d_refine + 3 * npix : nullptr;
    if (refine
        && (rc = sgm_launch_refine(w, &prof, d_main, mw, mh, d_map, witness,
                C.n_neighbors + C.n_witness, *C.photo, *C.refine, d_refine, d_map,
                C.slant != nullptr ? d_slant : nullptr, d_confidence, d_views)) != SMVS_OK)
        return rc;
    if (photo && !refine
        && (rc = sgm_launch_photo(w, &prof, d_main, mw, mh, d_map, witness,
                C.n_neighbors + C.n_witness, *C.photo, d_map,
                C.confidence != nullptr ? d_confidence : nullptr,
                C.views != nullptr ? d_views : nullptr)) != SMVS_OK)
        return rc;
    if (sgm_speckle_on(C.filter)
        && (rc = sgm_launch_speckle(w, &prof, d_map, mw, mh, C.filter->speckle_size,
                C.filter->speckle_ratio, d_speckle, d_map, false)) != SMVS_OK)
        return rc;
    auto get = [&w](void *host, const void *dev, size_t bytes) {
        return host != nullptr ? w.download(host, dev, bytes) : (int)SMVS_OK;
    };
    if (photo && ((rc = get(C.confidence, d_confidence, sizeof(float) * npix))
            || (rc = get(C.views, d_views, npix))
            || (refine && (rc = get(C.slant, d_slant, 2 * sizeof(float) * npix)))))
        return rc;
    // the consensus's own outputs, then the map (every download waits for the
    // stream: nothing is left to synchronise)
    if (!C.sweep)
        return (rc = get(C.checked, d_checked, sizeof(float) * npix * (size_t)C.n_neighbors))
                || (rc = get(C.support, d_support, npix))
            ? rc : get(C.depth, d_map, sizeof(float) * npix);
    size_t const vol = npix * (size_t)C.P.num_steps;
    if ((rc = get(C.depth, d_map, sizeof(float) * npix))
        || (rc = get(C.runner_up, B.runner_up, sizeof(uint16_t) * npix))
        || (rc = get(C.argmin, B.argmin, sizeof(int32_t) * npix))
        || (rc = get(C.support, d_support, npix))
        || (rc = get(C.sgm, B.sgm, sizeof(uint16_t) * vol))
        || (C.cost != nullptr && (rc = sgm_download_cost16(w, B.cost, vol, C.cost))))
        return rc;
    SMVS_HIP_CHECK(hipStreamSynchronize(w.stream));
    return SMVS_OK;
}

// -------------------------------------------------------------- the fronts
// reconstruct_sgm_depth_for_view: both neighbour images prepared before the
// first run (every buffer before the first SGM launch: growing one waits for
// the stream); per neighbour the two runs and the left/right check; the merge.
static int
sgm_front_reference(SgmViewSession &S, SgmViewCall const &C)
{
    int rc;
    Workspace &ws = S.ws();
    int const n = C.n_neighbors, mw = S.mw, mh = S.mh;
    size_t const npix = S.npix;
    uint8_t *d_nbr[2] = { nullptr, nullptr };
    int nw[2] = { 0, 0 }, nh[2] = { 0, 0 };
    for (int k = 0; k < n; ++k)
        if ((rc = S.neighbor(k, k == 0 ? WS_NBR0 : WS_NBR1, k == 0 ? WS_RAW0 : WS_RAW1,
                 &d_nbr[k], &nw[k], &nh[k])) != SMVS_OK)
            return rc;
    float *d_fwd[2] = { nullptr, nullptr }, *d_bwd = nullptr;
    size_t max_nnpix = 0;
    for (int k = 0; k < n; ++k) {
        size_t const nnpix = (size_t)nw[k] * nh[k];
        max_nnpix = nnpix > max_nnpix ? nnpix : max_nnpix;
        if ((rc = ws.ensure(k == 0 ? WS_FWD0 : WS_FWD1, npix, &d_fwd[k])))
            return rc;
    }
    if ((rc = ws.ensure(WS_BWD, max_nnpix, &d_bwd))
        || (rc = S.ensure_runs(npix > max_nnpix ? npix : max_nnpix)))
        return rc;
    for (int k = 0; k < n; ++k) {
        if ((rc = S.run_pair(k, d_nbr[k], nw[k], nh[k], d_fwd[k], d_bwd)) != SMVS_OK)
            return rc;
        LrArgs const L = fill_lr_args(d_fwd[k], d_bwd, mw, mh, nw[k], nh[k],
            C.neighbors[k].M_fwd, C.neighbors[k].t_fwd);
        {
            SgmKernelTimer timer(&S.prof, ws.stream, SMVS_SGM_K_LR_CHECK);
            hipLaunchKernelGGL(sgm_lr_check_kernel, dim3((mw + 255) / 256, mh),
                dim3(256), 0, ws.stream, L);
        }
        SMVS_HIP_CHECK(hipGetLastError());
    }
    if (n > 1) {
        SgmKernelTimer timer(&S.prof, ws.stream, SMVS_SGM_K_MERGE);
        hipLaunchKernelGGL(sgm_merge_kernel, dim3((unsigned)((npix + 255) / 256)),
            dim3(256), 0, ws.stream, d_fwd[0], d_fwd[1], npix);
        SMVS_HIP_CHECK(hipGetLastError());
    }
    return S.finish(d_fwd[0], nullptr, nullptr);
}

// SMVS_SGM_MERGE_CONSENSUS: 2 n runs, the neighbour images one at a time
// through the slots of neighbour 0, the n forward and n backward maps kept,
// then the fused kernel.
static int
sgm_front_consensus(SgmViewSession &S, SgmViewCall const &C)
{
    int rc;
    Workspace &ws = S.ws();
    int const n = C.n_neighbors, mw = S.mw, mh = S.mh;
    size_t const npix = S.npix;
    size_t bwd_at[SMVS_MAX_SUBS + 1] = { 0 };
    size_t max_nnpix = 0, max_out = 0, max_tmp = 0;
    for (int k = 0; k < n; ++k) {
        SgmPreparedSize const Z = sgm_prepared_size(C.neighbors[k].width, C.neighbors[k].height,
            C.neighbor_channels[k], C.halvings);
        size_t const nnpix = (size_t)Z.w * Z.h;
        max_out = Z.out > max_out ? Z.out : max_out;
        max_tmp = Z.tmp > max_tmp ? Z.tmp : max_tmp;
        max_nnpix = nnpix > max_nnpix ? nnpix : max_nnpix;
        bwd_at[k + 1] = bwd_at[k] + nnpix;
    }
    // every buffer at its largest size before the first SGM launch (growing one
    // waits for the stream): the neighbours' slots, the maps, the volumes
    uint8_t *d_nbr = nullptr, *d_tmp = nullptr, *d_support = nullptr;
    float *d_fwd = nullptr, *d_bwd = nullptr, *d_merged = nullptr;
    if ((rc = ws.ensure(WS_NBR0, max_out, &d_nbr))
        || (max_tmp != 0 && (rc = ws.ensure(WS_RAW0, max_tmp, &d_tmp)))
        || (rc = ws.ensure(WS_FWDN, npix * (size_t)n, &d_fwd))
        || (rc = ws.ensure(WS_BWDN, bwd_at[n], &d_bwd))
        || (rc = ws.ensure(WS_FWD0, npix, &d_merged))
        || (rc = ws.ensure(WS_SUPPORT, npix, &d_support))
        || (rc = S.ensure_runs(npix > max_nnpix ? npix : max_nnpix)))
        return rc;
    CheckMergeArgs A;
    for (int k = 0; k < n; ++k) {
        int pw = 0, ph = 0;
        if ((rc = S.neighbor(k, WS_NBR0, WS_RAW0, &d_nbr, &pw, &ph)) != SMVS_OK
            || (rc = S.run_pair(k, d_nbr, pw, ph, d_fwd + npix * (size_t)k, d_bwd + bwd_at[k]))
                != SMVS_OK)
            return rc;
        fill_check_neighbor(&A.nb[k], d_bwd + bwd_at[k], pw, ph, C.neighbors[k].M_fwd,
            C.neighbors[k].t_fwd);
    }
    fill_check_merge(&A, n, d_fwd, d_merged, C.checked != nullptr,
        C.support != nullptr ? d_support : nullptr, mw, mh, C.view_opts.min_agree,
        C.view_opts.agree_ratio);
    if ((rc = launch_check_merge(A, n, &S.prof, ws.stream)) != SMVS_OK)
        return rc;
    return S.finish(d_merged, d_fwd, d_support);
}

// (declared in sgm_internal.h)
int
sgm_run_view_call(SgmViewCall const &C)
{
    int rc;
    if ((rc = check_sgm_view_call(C)) != SMVS_OK)
        return rc;
    SgmViewSession S(C);
    if ((rc = S.open()) != SMVS_OK)
        return rc;
    if (C.sweep)
        return sgm_front_sweep(S, C);
    return C.view_opts.merge == SMVS_SGM_MERGE_CONSENSUS ? sgm_front_consensus(S, C)
                                               : sgm_front_reference(S, C);
}

} // namespace smvs_hip

using namespace smvs_hip;

// ------------------------------------------------------------- the entries
// Two entries fill a record: the one that takes smvs_sgm_options and the one
// that takes smvs_sgm_view_options with the filters, the photo test and the
// refinement sweeps, both on raw images.  The others are one of the two with the
// fields they do not take set to what they mean: the reference's constant
// penalty2 and plane winner, one channel at SGM scale, both filters off, the
// photo test off, the refinement off.
extern "C" int
smvs_sgm_depth_for_view_raw_opts(int device, const uint8_t *main_img, int w, int h,
    int channels, const smvs_sgm_neighbor *neighbors, const int *neighbor_channels,
    int n_neighbors, int halvings, int num_steps, uint16_t penalty1,
    uint16_t penalty2, const smvs_sgm_options *opts, float *depth)
{
    smvs_sgm_options const o = opts != nullptr ? *opts : smvs_sgm_options{};
    SgmViewCall const C = { .device = device, .main_img = main_img, .w = w, .h = h,
        .channels = channels, .neighbors = neighbors, .neighbor_channels = neighbor_channels,
        .n_neighbors = n_neighbors, .halvings = halvings,
        .P = { num_steps, penalty1, penalty2, o.p2_mode, o.winner },
        .view_opts = { o.p2_mode, o.winner, SMVS_SGM_MERGE_REFERENCE, 0, 0.0f },
        .filter = &SGM_FILTERS_OFF,
        .null_options = opts != nullptr ? nullptr : "null options (winner, p2_mode)",
        .depth = depth, .photo = &SGM_PHOTO_OFF, .refine = &SGM_REFINE_OFF };
    return sgm_run_view_call(C);
}

extern "C" int
smvs_sgm_depth_for_view_raw_refine(int device, const uint8_t *main_img, int w, int h,
    int channels, const smvs_sgm_neighbor *neighbors, const int *neighbor_channels,
    int n_neighbors, int halvings, int num_steps, uint16_t penalty1,
    uint16_t penalty2, const smvs_sgm_view_options *opts,
    const smvs_sgm_filter_options *filter, float *depth, float *checked, uint8_t *support,
    int n_witness, const smvs_sgm_photo_options *photo, float *confidence, uint8_t *views,
    const smvs_sgm_refine_options *refine, float *slant)
{
    smvs_sgm_view_options const o = opts != nullptr ? *opts : smvs_sgm_view_options{};
    SgmViewCall const C = { .device = device, .main_img = main_img, .w = w, .h = h,
        .channels = channels, .neighbors = neighbors, .neighbor_channels = neighbor_channels,
        .n_neighbors = n_neighbors, .halvings = halvings,
        .P = { num_steps, penalty1, penalty2, o.p2_mode, o.winner }, .view_opts = o,
        .filter = filter,
        .null_options = opts != nullptr ? nullptr : "null options (p2_mode, winner, merge)",
        .depth = depth, .checked = checked, .support = support, .n_witness = n_witness,
        .photo = photo, .confidence = confidence, .views = views, .refine = refine,
        .slant = slant };
    return sgm_run_view_call(C);
}

extern "C" int
smvs_sgm_depth_for_view_raw_photo(int device, const uint8_t *main_img, int w, int h,
    int channels, const smvs_sgm_neighbor *neighbors, const int *neighbor_channels,
    int n_neighbors, int halvings, int num_steps, uint16_t penalty1,
    uint16_t penalty2, const smvs_sgm_view_options *opts,
    const smvs_sgm_filter_options *filter, float *depth, float *checked, uint8_t *support,
    int n_witness, const smvs_sgm_photo_options *photo, float *confidence, uint8_t *views)
{
    return smvs_sgm_depth_for_view_raw_refine(device, main_img, w, h, channels, neighbors,
        neighbor_channels, n_neighbors, halvings, num_steps, penalty1, penalty2, opts, filter,
        depth, checked, support, n_witness, photo, confidence, views, &SGM_REFINE_OFF, nullptr);
}

extern "C" int
smvs_sgm_depth_for_view_raw_filtered(int device, const uint8_t *main_img, int w, int h,
    int channels, const smvs_sgm_neighbor *neighbors, const int *neighbor_channels,
    int n_neighbors, int halvings, int num_steps, uint16_t penalty1,
    uint16_t penalty2, const smvs_sgm_view_options *opts,
    const smvs_sgm_filter_options *filter, float *depth, float *checked, uint8_t *support)
{
    return smvs_sgm_depth_for_view_raw_photo(device, main_img, w, h, channels, neighbors,
        neighbor_channels, n_neighbors, halvings, num_steps, penalty1, penalty2, opts, filter,
        depth, checked, support, 0, &SGM_PHOTO_OFF, nullptr, nullptr);
}

// sgm_stereo.cc:274-306 with opts->winner = SMVS_SGM_WINNER_SUBPLANE in all four
// runs of the view
extern "C" int
smvs_sgm_depth_for_view_opts(int device, const uint8_t *main_img, int w, int h,
    const smvs_sgm_neighbor *neighbors, int n_neighbors, int num_steps,
    uint16_t penalty1, uint16_t penalty2, const smvs_sgm_options *opts, float *depth)
{
    return smvs_sgm_depth_for_view_raw_opts(device, main_img, w, h, 1, neighbors,
        SGM_ONE_CHANNEL, n_neighbors, 0, num_steps, penalty1, penalty2, opts, depth);
}

// sgm_stereo.cc:310-346 with p2_mode = SMVS_SGM_P2_ADAPTIVE
extern "C" int
smvs_sgm_depth_for_view_mode(int device, const uint8_t *main_img, int w, int h,
    const smvs_sgm_neighbor *neighbors, int n_neighbors, int num_steps,
    uint16_t penalty1, uint16_t penalty2, int p2_mode, float *depth)
{
    smvs_sgm_options const opts = { p2_mode, SMVS_SGM_WINNER_PLANE };
    return smvs_sgm_depth_for_view_opts(device, main_img, w, h, neighbors, n_neighbors,
        num_steps, penalty1, penalty2, &opts, depth);
}

extern "C" int
smvs_sgm_depth_for_view(int device, const uint8_t *main_img, int w, int h,
    const smvs_sgm_neighbor *neighbors, int n_neighbors, int num_steps,
    uint16_t penalty1, uint16_t penalty2, float *depth)
{
    return smvs_sgm_depth_for_view_mode(device, main_img, w, h, neighbors, n_neighbors,
        num_steps, penalty1, penalty2, SMVS_SGM_P2_CONSTANT, depth);
}

// sgm_stereo.cc:310-346 with p2_mode = SMVS_SGM_P2_ADAPTIVE
extern "C" int
smvs_sgm_depth_for_view_raw_mode(int device, const uint8_t *main_img, int w, int h,
    int channels, const smvs_sgm_neighbor *neighbors, const int *neighbor_channels,
    int n_neighbors, int halvings, int num_steps, uint16_t penalty1,
    uint16_t penalty2, int p2_mode, float *depth)
{
    smvs_sgm_options const opts = { p2_mode, SMVS_SGM_WINNER_PLANE };
    return smvs_sgm_depth_for_view_raw_opts(device, main_img, w, h, channels, neighbors,
        neighbor_channels, n_neighbors, halvings, num_steps, penalty1, penalty2, &opts,
        depth);
}

extern "C" int
smvs_sgm_depth_for_view_raw(int device, const uint8_t *main_img, int w, int h,
    int channels, const smvs_sgm_neighbor *neighbors, const int *neighbor_channels,
    int n_neighbors, int halvings, int num_steps, uint16_t penalty1,
    uint16_t penalty2, float *depth)
{
    return smvs_sgm_depth_for_view_raw_mode(device, main_img, w, h, channels, neighbors,
        neighbor_channels, n_neighbors, halvings, num_steps, penalty1, penalty2,
        SMVS_SGM_P2_CONSTANT, depth);
}

extern "C" int
smvs_sgm_depth_for_view_raw_merge(int device, const uint8_t *main_img, int w, int h,
    int channels, const smvs_sgm_neighbor *neighbors, const int *neighbor_channels,
    int n_neighbors, int halvings, int num_steps, uint16_t penalty1,
    uint16_t penalty2, const smvs_sgm_view_options *opts, float *depth, float *checked,
    uint8_t *support)
{
    return smvs_sgm_depth_for_view_raw_filtered(device, main_img, w, h, channels, neighbors,
        neighbor_channels, n_neighbors, halvings, num_steps, penalty1, penalty2, opts,
        &SGM_FILTERS_OFF, depth, checked, support);
}

// smvs_sgm_depth_for_view_merge with the uniqueness test in every run of the
// view and the speckle filter on the merged map
extern "C" int
smvs_sgm_depth_for_view_filtered(int device, const uint8_t *main_img, int w, int h,
    const smvs_sgm_neighbor *neighbors, int n_neighbors, int num_steps,
    uint16_t penalty1, uint16_t penalty2, const smvs_sgm_view_options *opts,
    const smvs_sgm_filter_options *filter, float *depth, float *checked, uint8_t *support)
{
    return smvs_sgm_depth_for_view_raw_filtered(device, main_img, w, h, 1, neighbors,
        SGM_ONE_CHANNEL, n_neighbors, 0, num_steps, penalty1, penalty2, opts, filter, depth,
        checked, support);
}

extern "C" int
smvs_sgm_depth_for_view_merge(int device, const uint8_t *main_img, int w, int h,
    const smvs_sgm_neighbor *neighbors, int n_neighbors, int num_steps,
    uint16_t penalty1, uint16_t penalty2, const smvs_sgm_view_options *opts,
    float *depth, float *checked, uint8_t *support)
{
    return smvs_sgm_depth_for_view_filtered(device, main_img, w, h, neighbors, n_neighbors,
        num_steps, penalty1, penalty2, opts, &SGM_FILTERS_OFF, depth, checked, support);
}

// the fused kernel alone, on the caller's maps
extern "C" int
smvs_sgm_check_merge(int device, const float *fwd, int w, int h,
    const smvs_sgm_check_neighbor *neighbors, int n_neighbors,
    const smvs_sgm_view_options *opts, float *merged, float *checked, uint8_t *support)
{
    SMVS_REQUIRE(opts != nullptr, "null options (merge, min_agree, agree_ratio)");
    SMVS_REQUIRE(opts->merge == SMVS_SGM_MERGE_CONSENSUS,
        "smvs_sgm_check_merge is the consensus merge");
    smvs_sgm_view_options o = *opts;
    o.winner = SMVS_SGM_WINNER_PLANE;       // (not read; any value is accepted)
    if (int const rc = check_sgm_view_options(&o, n_neighbors); rc != SMVS_OK)
        return rc;
    SMVS_REQUIRE(fwd && neighbors, "null argument");
    SMVS_REQUIRE(w >= 1 && h >= 1 && (size_t)w * h < ((size_t)1 << 31), "bad map size");
    size_t bwd_at[SMVS_MAX_SUBS + 1] = { 0 };
    for (int k = 0; k < n_neighbors; ++k) {
        SMVS_REQUIRE(neighbors[k].bwd && neighbors[k].width >= 1 && neighbors[k].height >= 1
                && (size_t)neighbors[k].width * neighbors[k].height < ((size_t)1 << 31),
            "bad neighbour map");
        bwd_at[k + 1] = bwd_at[k] + (size_t)neighbors[k].width * neighbors[k].height;
    }
    int rc;
    WorkspaceLease lease(device);
    if (lease.w == nullptr)
        return SMVS_ERR_HIP;
    Workspace &ws = *lease.w;
    SgmProfile prof;
    size_t const npix = (size_t)w * h;
    float *d_fwd = nullptr, *d_bwd = nullptr, *d_merged = nullptr;
    uint8_t *d_support = nullptr;
    if ((rc = ws.ensure(WS_FWDN, npix * (size_t)n_neighbors, &d_fwd))
        || (rc = ws.ensure(WS_BWDN, bwd_at[n_neighbors], &d_bwd))
        || (rc = ws.ensure(WS_FWD0, npix, &d_merged))
        || (rc = ws.ensure(WS_SUPPORT, npix, &d_support))
        || (rc = ws.upload(d_fwd, fwd, sizeof(float) * npix * (size_t)n_neighbors)))
        return rc;
    CheckMergeArgs A;
    for (int k = 0; k < n_neighbors; ++k) {
        smvs_sgm_check_neighbor const &N = neighbors[k];
        if ((rc = ws.upload(d_bwd + bwd_at[k], N.bwd,
                 sizeof(float) * (bwd_at[k + 1] - bwd_at[k]))))
            return rc;
        fill_check_neighbor(&A.nb[k], d_bwd + bwd_at[k], N.width, N.height, N.M_fwd, N.t_fwd);
    }
    fill_check_merge(&A, n_neighbors, d_fwd, d_merged, checked != nullptr, d_support, w, h,
        o.min_agree, o.agree_ratio);
    if ((rc = launch_check_merge(A, n_neighbors, &prof, ws.stream)) != SMVS_OK)
        return rc;
    if (checked != nullptr
        && (rc = ws.download(checked, d_fwd, sizeof(float) * npix * (size_t)n_neighbors)))
        return rc;
    if (support != nullptr && (rc = ws.download(support, d_support, npix)))
        return rc;
    if (merged != nullptr && (rc = ws.download(merged, d_merged, sizeof(float) * npix)))
        return rc;
    SMVS_HIP_CHECK(hipStreamSynchronize(ws.stream));
    return SMVS_OK;
}
