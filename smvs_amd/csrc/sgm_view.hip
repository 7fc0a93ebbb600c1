// A view's SGM front end on gfx950: SGMStereo::reconstruct (reference:
// lib/sgm_stereo.cc:46-91) -- run_sgm main -> neighbour and back (sgm.hip), the
// left/right consistency check -- and the two-neighbour merge of
// reconstruct_sgm_depth_for_view (app/smvsrecon.cc:360-377), on images that
// image_prep.hip brought to SGM scale.
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

} // namespace smvs_hip

using namespace smvs_hip;

// reconstruct_sgm_depth_for_view on prepared device images
static int
sgm_depth_for_view_impl(int device, const uint8_t *main_img, int w, int h,
    int main_channels, const smvs_sgm_neighbor *neighbors,
    const int *neighbor_channels, int n_neighbors, int halvings, int num_steps,
    uint16_t penalty1, uint16_t penalty2, int p2_mode, int winner, float *depth)
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
    WorkspaceLease lease(device);
    if (lease.w == nullptr)
        return SMVS_ERR_HIP;
    Workspace &ws = *lease.w;
    hipStream_t const stream = ws.stream;
    SgmProfile prof;
    SgmWorkspace B(&ws);
    B.prof = &prof;
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
                N.M_fwd, N.t_fwd, N.range_main[0], N.range_main[1], num_steps,
                penalty1, penalty2, p2_mode, winner, d_fwd[k])) != SMVS_OK)
            return rc;
        if ((rc = sgm_run_device(B, d_nbr[k], nw[k], nh[k], d_main, mw, mh,
                N.M_bwd, N.t_bwd, N.range_neighbor[0], N.range_neighbor[1],
                num_steps, penalty1, penalty2, p2_mode, winner, d_bwd)) != SMVS_OK)
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

