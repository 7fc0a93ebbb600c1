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

static void
fill_check_neighbor(CheckNeighbor *C, const float *d_bwd, int nw, int nh, const float *M,
    const float *t)
{
    C->bwd = d_bwd;
    C->nw = nw;
    C->nh = nh;
    C->cut = (int)(0.03 * (double)(nw > nh ? nw : nh));
    C->pad = 0;
    for (int i = 0; i < 9; ++i)
        C->M[i] = (double)M[i];
    for (int i = 0; i < 3; ++i)
        C->t[i] = (double)t[i];
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

} // namespace smvs_hip

using namespace smvs_hip;

// reconstruct_sgm_depth_for_view on prepared device images
static int
sgm_depth_for_view_impl(int device, const uint8_t *main_img, int w, int h,
    int main_channels, const smvs_sgm_neighbor *neighbors,
    const int *neighbor_channels, int n_neighbors, int halvings, int num_steps,
    uint16_t penalty1, uint16_t penalty2, int p2_mode, int winner, float *depth,
    const smvs_sgm_filter_options *filter = nullptr)
{
    SMVS_REQUIRE(p2_mode == SMVS_SGM_P2_CONSTANT || p2_mode == SMVS_SGM_P2_ADAPTIVE,
        "unknown penalty2 mode");
    if (p2_mode != SMVS_SGM_P2_CONSTANT) {
        int const prc = check_sgm_penalties(penalty1, penalty2, p2_mode);
        if (prc != SMVS_OK)
            return prc;
    }
    // (before the first device call, as the penalties: sgm_run_device checks
    // both again)
    if (int const src = check_sgm_plane_count(num_steps); src != SMVS_OK)
        return src;
    SMVS_REQUIRE(main_img && neighbors && depth, "null argument");
    SMVS_REQUIRE(n_neighbors >= 1 && n_neighbors <= 2,
        "one or two neighbours (app/smvsrecon.cc:360-365)");
    SMVS_REQUIRE(halvings >= 0 && halvings <= 8, "halvings out of range");
    SMVS_REQUIRE((w >> halvings) > 10 && (h >> halvings) > 8, "image too small");
    for (int k = 0; k < n_neighbors; ++k)
        SMVS_REQUIRE(neighbors[k].image && (neighbors[k].width >> halvings) > 10
            && (neighbors[k].height >> halvings) > 8, "bad neighbour image");
    int rc;
    SgmRunParams const P = { num_steps, penalty1, penalty2, p2_mode, winner };
    WorkspaceLease lease(device);
    if (lease.w == nullptr)
        return SMVS_ERR_HIP;
    Workspace &ws = *lease.w;
    hipStream_t const stream = ws.stream;
    SgmProfile prof;
    SgmWorkspace B(&ws);
    B.prof = &prof;
    B.set_filter(filter);
    // the SGM-scale images (every buffer before the first SGM launch: growing
    // one waits for the stream)
    uint8_t *d_main = nullptr, *d_nbr[2] = { nullptr, nullptr };
    int mw = 0, mh = 0, nw[2] = { 0, 0 }, nh[2] = { 0, 0 };
    if ((rc = sgm_prepare_image(ws, main_img, w, h, main_channels, halvings, WS_MAIN,
             WS_RAW, &d_main, &mw, &mh)) != SMVS_OK)
        return rc;
    for (int k = 0; k < n_neighbors; ++k)
        if ((rc = sgm_prepare_image(ws, neighbors[k].image, neighbors[k].width,
                 neighbors[k].height, neighbor_channels != nullptr ? neighbor_channels[k] : 1,
                 halvings, k == 0 ? WS_NBR0 : WS_NBR1, k == 0 ? WS_RAW0 : WS_RAW1,
                 &d_nbr[k], &nw[k], &nh[k])) != SMVS_OK)
            return rc;
    size_t const npix = (size_t)mw * mh;
    float *d_fwd[2] = { nullptr, nullptr }, *d_bwd = nullptr;
    uint32_t *d_speckle = nullptr;
    if (sgm_speckle_on(filter) && (rc = sgm_speckle_ensure(ws, npix, &d_speckle)))
        return rc;
    size_t max_nnpix = 0;
    for (int k = 0; k < n_neighbors; ++k) {
        size_t const nnpix = (size_t)nw[k] * nh[k];
        max_nnpix = nnpix > max_nnpix ? nnpix : max_nnpix;
        if ((rc = ws.ensure(k == 0 ? WS_FWD0 : WS_FWD1, npix, &d_fwd[k])))
            return rc;
    }
    if ((rc = ws.ensure(WS_BWD, max_nnpix, &d_bwd))
        || (rc = B.ensure(npix > max_nnpix ? npix : max_nnpix, num_steps,
                sgm_path_plan_here(num_steps,
                    SgmWorkspace::largest_penalty2(penalty1, penalty2, p2_mode)))))
        return rc;
    for (int k = 0; k < n_neighbors; ++k) {
        smvs_sgm_neighbor const &N = neighbors[k];
        // SGMStereo::reconstruct, sgm_stereo.cc:46-62: main -> neighbour,
        // then neighbour -> main with the neighbour's own depth range
        if ((rc = sgm_run_device(B, d_main, mw, mh, d_nbr[k], nw[k], nh[k],
                N.M_fwd, N.t_fwd, N.range_main[0], N.range_main[1], P, d_fwd[k])) != SMVS_OK)
            return rc;
        if ((rc = sgm_run_device(B, d_nbr[k], nw[k], nh[k], d_main, mw, mh,
                N.M_bwd, N.t_bwd, N.range_neighbor[0], N.range_neighbor[1], P, d_bwd))
            != SMVS_OK)
            return rc;
        LrArgs L;
        L.d_main = d_fwd[k];
        L.d_neig = d_bwd;
        L.w = mw;
        L.h = mh;
        L.nw = nw[k];
        L.nh = nh[k];
        L.cut = (int)(0.03 * (double)(nw[k] > nh[k] ? nw[k] : nh[k]));
        for (int i = 0; i < 9; ++i)
            L.M[i] = (double)N.M_fwd[i];
        for (int i = 0; i < 3; ++i)
            L.t[i] = (double)N.t_fwd[i];
        {
            SgmKernelTimer timer(&prof, stream, SMVS_SGM_K_LR_CHECK);
            hipLaunchKernelGGL(sgm_lr_check_kernel, dim3((mw + 255) / 256, mh),
                dim3(256), 0, stream, L);
        }
        SMVS_HIP_CHECK(hipGetLastError());
    }
    if (n_neighbors > 1) {
        SgmKernelTimer timer(&prof, stream, SMVS_SGM_K_MERGE);
        hipLaunchKernelGGL(sgm_merge_kernel, dim3((unsigned)((npix + 255) / 256)),
            dim3(256), 0, stream, d_fwd[0], d_fwd[1], npix);
        SMVS_HIP_CHECK(hipGetLastError());
    }
    if (sgm_speckle_on(filter)
        && (rc = sgm_launch_speckle(ws, &prof, d_fwd[0], mw, mh, filter->speckle_size,
                filter->speckle_ratio, d_speckle, d_fwd[0], false)) != SMVS_OK)
        return rc;
    return ws.download(depth, d_fwd[0], sizeof(float) * npix);
}

extern "C" int
smvs_sgm_depth_for_view(int device, const uint8_t *main_img, int w, int h,
    const smvs_sgm_neighbor *neighbors, int n_neighbors, int num_steps,
    uint16_t penalty1, uint16_t penalty2, float *depth)
{
    return sgm_depth_for_view_impl(device, main_img, w, h, 1, neighbors, nullptr,
        n_neighbors, 0, num_steps, penalty1, penalty2, SMVS_SGM_P2_CONSTANT,
        SMVS_SGM_WINNER_PLANE, depth);
}

// sgm_stereo.cc:310-346 with p2_mode = SMVS_SGM_P2_ADAPTIVE
extern "C" int
smvs_sgm_depth_for_view_mode(int device, const uint8_t *main_img, int w, int h,
    const smvs_sgm_neighbor *neighbors, int n_neighbors, int num_steps,
    uint16_t penalty1, uint16_t penalty2, int p2_mode, float *depth)
{
    return sgm_depth_for_view_impl(device, main_img, w, h, 1, neighbors, nullptr,
        n_neighbors, 0, num_steps, penalty1, penalty2, p2_mode, SMVS_SGM_WINNER_PLANE,
        depth);
}

// sgm_stereo.cc:274-306 with opts->winner = SMVS_SGM_WINNER_SUBPLANE in all four
// runs of the view
extern "C" int
smvs_sgm_depth_for_view_opts(int device, const uint8_t *main_img, int w, int h,
    const smvs_sgm_neighbor *neighbors, int n_neighbors, int num_steps,
    uint16_t penalty1, uint16_t penalty2, const smvs_sgm_options *opts, float *depth)
{
    if (int const rc = check_sgm_winner(opts); rc != SMVS_OK)
        return rc;
    return sgm_depth_for_view_impl(device, main_img, w, h, 1, neighbors, nullptr,
        n_neighbors, 0, num_steps, penalty1, penalty2, opts->p2_mode, opts->winner, depth);
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

// sgm_stereo.cc:274-306 with opts->winner = SMVS_SGM_WINNER_SUBPLANE in all four
// runs of the view
extern "C" int
smvs_sgm_depth_for_view_raw_opts(int device, const uint8_t *main_img, int w, int h,
    int channels, const smvs_sgm_neighbor *neighbors, const int *neighbor_channels,
    int n_neighbors, int halvings, int num_steps, uint16_t penalty1,
    uint16_t penalty2, const smvs_sgm_options *opts, float *depth)
{
    if (int const rc = check_sgm_winner(opts); rc != SMVS_OK)
        return rc;
    int const p2_mode = opts->p2_mode;
    SMVS_REQUIRE(p2_mode == SMVS_SGM_P2_CONSTANT || p2_mode == SMVS_SGM_P2_ADAPTIVE,
        "unknown penalty2 mode");
    SMVS_REQUIRE(channels == 1 || channels == 3, "1 or 3 channels");
    SMVS_REQUIRE(neighbor_channels != nullptr, "null argument");
    for (int k = 0; k < n_neighbors && k < 2; ++k)
        SMVS_REQUIRE(neighbor_channels[k] == 1 || neighbor_channels[k] == 3,
            "1 or 3 channels");
    return sgm_depth_for_view_impl(device, main_img, w, h, channels, neighbors,
        neighbor_channels, n_neighbors, halvings, num_steps, penalty1, penalty2, p2_mode,
        opts->winner, depth);
}


// The front end with SMVS_SGM_MERGE_CONSENSUS: 2 n runs, the neighbour images
// one at a time through the slots of neighbour 0, the n forward and n backward
// maps kept, then the fused kernel.
static int
sgm_depth_for_view_consensus(int device, const uint8_t *main_img, int w, int h,
    int main_channels, const smvs_sgm_neighbor *neighbors, const int *neighbor_channels,
    int n_neighbors, int halvings, int num_steps, uint16_t penalty1, uint16_t penalty2,
    const smvs_sgm_view_options *opts, float *depth, float *checked, uint8_t *support,
    const smvs_sgm_filter_options *filter = nullptr)
{
    int const p2_mode = opts->p2_mode;
    SgmRunParams const P = { num_steps, penalty1, penalty2, p2_mode, opts->winner };
    int rc;
    if ((rc = check_sgm_penalties(penalty1, penalty2, p2_mode)) != SMVS_OK
        || (rc = check_sgm_plane_count(num_steps)) != SMVS_OK)
        return rc;
    SMVS_REQUIRE(main_img && neighbors && depth, "null argument");
    SMVS_REQUIRE(halvings >= 0 && halvings <= 8, "halvings out of range");
    SMVS_REQUIRE((w >> halvings) > 10 && (h >> halvings) > 8, "image too small");
    // the SGM-scale sizes ((s + 1) >> 1 per halving, as sgm_prepare_image)
    int nw[SMVS_MAX_SUBS], nh[SMVS_MAX_SUBS];
    size_t bwd_at[SMVS_MAX_SUBS + 1] = { 0 };
    size_t max_nnpix = 0, max_rawpix = 0, max_tmp = 0;
    for (int k = 0; k < n_neighbors; ++k) {
        smvs_sgm_neighbor const &N = neighbors[k];
        SMVS_REQUIRE(N.image && (N.width >> halvings) > 10 && (N.height >> halvings) > 8,
            "bad neighbour image");
        int const ch = neighbor_channels != nullptr ? neighbor_channels[k] : 1;
        // (what sgm_prepare_image asks of its two slots)
        size_t const rawpix = (size_t)N.width * N.height;
        size_t const tmp = ch == 1 && halvings == 0 ? 0 : rawpix * (size_t)(ch + 1);
        max_rawpix = rawpix > max_rawpix ? rawpix : max_rawpix;
        max_tmp = tmp > max_tmp ? tmp : max_tmp;
        nw[k] = N.width;
        nh[k] = N.height;
        for (int i = 0; i < halvings; ++i) {
            nw[k] = (nw[k] + 1) >> 1;
            nh[k] = (nh[k] + 1) >> 1;
        }
        size_t const nnpix = (size_t)nw[k] * nh[k];
        max_nnpix = nnpix > max_nnpix ? nnpix : max_nnpix;
        bwd_at[k + 1] = bwd_at[k] + nnpix;
    }
    WorkspaceLease lease(device);
    if (lease.w == nullptr)
        return SMVS_ERR_HIP;
    Workspace &ws = *lease.w;
    hipStream_t const stream = ws.stream;
    SgmProfile prof;
    SgmWorkspace B(&ws);
    B.prof = &prof;
    B.set_filter(filter);
    uint8_t *d_main = nullptr, *d_nbr = nullptr, *d_tmp = nullptr;
    int mw = 0, mh = 0;
    if ((rc = sgm_prepare_image(ws, main_img, w, h, main_channels, halvings, WS_MAIN,
             WS_RAW, &d_main, &mw, &mh)) != SMVS_OK)
        return rc;
    size_t const npix = (size_t)mw * mh;
    // every buffer at its largest size before the first SGM launch (growing one
    // waits for the stream): the two slots all neighbour images pass through,
    // the maps, the volumes
    float *d_fwd = nullptr, *d_bwd = nullptr, *d_merged = nullptr;
    uint8_t *d_support = nullptr;
    uint32_t *d_speckle = nullptr;
    if (sgm_speckle_on(filter) && (rc = sgm_speckle_ensure(ws, npix, &d_speckle)))
        return rc;
    if ((rc = ws.ensure(WS_NBR0, max_rawpix, &d_nbr))
        || (max_tmp != 0 && (rc = ws.ensure(WS_RAW0, max_tmp, &d_tmp)))
        || (rc = ws.ensure(WS_FWDN, npix * (size_t)n_neighbors, &d_fwd))
        || (rc = ws.ensure(WS_BWDN, bwd_at[n_neighbors], &d_bwd))
        || (rc = ws.ensure(WS_FWD0, npix, &d_merged))
        || (rc = ws.ensure(WS_SUPPORT, npix, &d_support))
        || (rc = B.ensure(npix > max_nnpix ? npix : max_nnpix, num_steps,
                sgm_path_plan_here(num_steps,
                    SgmWorkspace::largest_penalty2(penalty1, penalty2, p2_mode)))))
        return rc;
    CheckMergeArgs A;
    for (int k = 0; k < n_neighbors; ++k) {
        smvs_sgm_neighbor const &N = neighbors[k];
        int pw = 0, ph = 0;
        if ((rc = sgm_prepare_image(ws, N.image, N.width, N.height,
                 neighbor_channels != nullptr ? neighbor_channels[k] : 1, halvings, WS_NBR0,
                 WS_RAW0, &d_nbr, &pw, &ph)) != SMVS_OK)
            return rc;
        SMVS_REQUIRE(pw == nw[k] && ph == nh[k], "SGM-scale size of a neighbour");
        // SGMStereo::reconstruct, sgm_stereo.cc:46-62, as in the reference's merge
        if ((rc = sgm_run_device(B, d_main, mw, mh, d_nbr, pw, ph, N.M_fwd, N.t_fwd,
                N.range_main[0], N.range_main[1], P, d_fwd + npix * (size_t)k)) != SMVS_OK)
            return rc;
        if ((rc = sgm_run_device(B, d_nbr, pw, ph, d_main, mw, mh, N.M_bwd, N.t_bwd,
                N.range_neighbor[0], N.range_neighbor[1], P, d_bwd + bwd_at[k])) != SMVS_OK)
            return rc;
        fill_check_neighbor(&A.nb[k], d_bwd + bwd_at[k], pw, ph, N.M_fwd, N.t_fwd);
    }
    for (int k = n_neighbors; k < SMVS_MAX_SUBS; ++k)
        A.nb[k] = A.nb[0];
    A.fwd = d_fwd;
    A.merged = d_merged;
    A.checked = checked != nullptr ? d_fwd : nullptr;      // in place
    A.support = support != nullptr ? d_support : nullptr;
    A.w = mw;
    A.h = mh;
    A.min_agree = opts->min_agree;
    A.agree_ratio = opts->agree_ratio;
    if ((rc = launch_check_merge(A, n_neighbors, &prof, stream)) != SMVS_OK)
        return rc;
    // (checked and support are those of the merge: the speckle filter sees the
    // merged map only)
    if (sgm_speckle_on(filter)
        && (rc = sgm_launch_speckle(ws, &prof, d_merged, mw, mh, filter->speckle_size,
                filter->speckle_ratio, d_speckle, d_merged, false)) != SMVS_OK)
        return rc;
    if (checked != nullptr
        && (rc = ws.download(checked, d_fwd, sizeof(float) * npix * (size_t)n_neighbors)))
        return rc;
    if (support != nullptr && (rc = ws.download(support, d_support, npix)))
        return rc;
    return ws.download(depth, d_merged, sizeof(float) * npix);
}

// (filter: null in the entries without the filters)
static int
sgm_depth_for_view_merge_impl(int device, const uint8_t *main_img, int w, int h,
    const smvs_sgm_neighbor *neighbors, int n_neighbors, int num_steps,
    uint16_t penalty1, uint16_t penalty2, const smvs_sgm_view_options *opts,
    const smvs_sgm_filter_options *filter, float *depth, float *checked, uint8_t *support)
{
    if (int const rc = check_sgm_view_options(opts, n_neighbors); rc != SMVS_OK)
        return rc;
    if (opts->merge == SMVS_SGM_MERGE_REFERENCE) {
        SMVS_REQUIRE(checked == nullptr && support == nullptr,
            "checked and support are outputs of the consensus merge");
        return sgm_depth_for_view_impl(device, main_img, w, h, 1, neighbors, nullptr,
            n_neighbors, 0, num_steps, penalty1, penalty2, opts->p2_mode, opts->winner,
            depth, filter);
    }
    return sgm_depth_for_view_consensus(device, main_img, w, h, 1, neighbors, nullptr,
        n_neighbors, 0, num_steps, penalty1, penalty2, opts, depth, checked, support, filter);
}

extern "C" int
smvs_sgm_depth_for_view_merge(int device, const uint8_t *main_img, int w, int h,
    const smvs_sgm_neighbor *neighbors, int n_neighbors, int num_steps,
    uint16_t penalty1, uint16_t penalty2, const smvs_sgm_view_options *opts,
    float *depth, float *checked, uint8_t *support)
{
    return sgm_depth_for_view_merge_impl(device, main_img, w, h, neighbors, n_neighbors,
        num_steps, penalty1, penalty2, opts, nullptr, depth, checked, support);
}

// smvs_sgm_depth_for_view_merge with the uniqueness test in every run of the
// view and the speckle filter on the merged map
extern "C" int
smvs_sgm_depth_for_view_filtered(int device, const uint8_t *main_img, int w, int h,
    const smvs_sgm_neighbor *neighbors, int n_neighbors, int num_steps,
    uint16_t penalty1, uint16_t penalty2, const smvs_sgm_view_options *opts,
    const smvs_sgm_filter_options *filter, float *depth, float *checked, uint8_t *support)
{
    if (int const rc = check_sgm_filter(filter, false); rc != SMVS_OK)
        return rc;
    return sgm_depth_for_view_merge_impl(device, main_img, w, h, neighbors, n_neighbors,
        num_steps, penalty1, penalty2, opts, filter, depth, checked, support);
}

static int
sgm_depth_for_view_raw_merge_impl(int device, const uint8_t *main_img, int w, int h,
    int channels, const smvs_sgm_neighbor *neighbors, const int *neighbor_channels,
    int n_neighbors, int halvings, int num_steps, uint16_t penalty1,
    uint16_t penalty2, const smvs_sgm_view_options *opts,
    const smvs_sgm_filter_options *filter, float *depth, float *checked, uint8_t *support)
{
    if (int const rc = check_sgm_view_options(opts, n_neighbors); rc != SMVS_OK)
        return rc;
    SMVS_REQUIRE(opts->p2_mode == SMVS_SGM_P2_CONSTANT
            || opts->p2_mode == SMVS_SGM_P2_ADAPTIVE, "unknown penalty2 mode");
    SMVS_REQUIRE(channels == 1 || channels == 3, "1 or 3 channels");
    SMVS_REQUIRE(neighbor_channels != nullptr, "null argument");
    for (int k = 0; k < n_neighbors; ++k)
        SMVS_REQUIRE(neighbor_channels[k] == 1 || neighbor_channels[k] == 3,
            "1 or 3 channels");
    if (opts->merge == SMVS_SGM_MERGE_REFERENCE) {
        SMVS_REQUIRE(checked == nullptr && support == nullptr,
            "checked and support are outputs of the consensus merge");
        return sgm_depth_for_view_impl(device, main_img, w, h, channels, neighbors,
            neighbor_channels, n_neighbors, halvings, num_steps, penalty1, penalty2,
            opts->p2_mode, opts->winner, depth, filter);
    }
    return sgm_depth_for_view_consensus(device, main_img, w, h, channels, neighbors,
        neighbor_channels, n_neighbors, halvings, num_steps, penalty1, penalty2, opts, depth,
        checked, support, filter);
}

extern "C" int
smvs_sgm_depth_for_view_raw_merge(int device, const uint8_t *main_img, int w, int h,
    int channels, const smvs_sgm_neighbor *neighbors, const int *neighbor_channels,
    int n_neighbors, int halvings, int num_steps, uint16_t penalty1,
    uint16_t penalty2, const smvs_sgm_view_options *opts, float *depth, float *checked,
    uint8_t *support)
{
    return sgm_depth_for_view_raw_merge_impl(device, main_img, w, h, channels, neighbors,
        neighbor_channels, n_neighbors, halvings, num_steps, penalty1, penalty2, opts, nullptr,
        depth, checked, support);
}

// smvs_sgm_depth_for_view_raw_merge with the filters
extern "C" int
smvs_sgm_depth_for_view_raw_filtered(int device, const uint8_t *main_img, int w, int h,
    int channels, const smvs_sgm_neighbor *neighbors, const int *neighbor_channels,
    int n_neighbors, int halvings, int num_steps, uint16_t penalty1,
    uint16_t penalty2, const smvs_sgm_view_options *opts,
    const smvs_sgm_filter_options *filter, float *depth, float *checked, uint8_t *support)
{
    if (int const rc = check_sgm_filter(filter, false); rc != SMVS_OK)
        return rc;
    return sgm_depth_for_view_raw_merge_impl(device, main_img, w, h, channels, neighbors,
        neighbor_channels, n_neighbors, halvings, num_steps, penalty1, penalty2, opts, filter,
        depth, checked, support);
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
    for (int k = n_neighbors; k < SMVS_MAX_SUBS; ++k)
        A.nb[k] = A.nb[0];
    A.fwd = d_fwd;
    A.merged = d_merged;
    A.checked = checked != nullptr ? d_fwd : nullptr;      // in place
    A.support = d_support;
    A.w = w;
    A.h = h;
    A.min_agree = o.min_agree;
    A.agree_ratio = o.agree_ratio;
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
