// Multi-view photo-consistency test on a depth map on gfx950 (not in the
// reference; include/smvs_hip.h, "Multi-view photo-consistency test", has the
// definition): per valid pixel and witness the (2 r + 1)^2 window of the main
// image against its warp into the witness at the pixel's own depth, the signed
// squared correlation of the two from integer sums, the mean of the best few
// witnesses as the pixel's confidence, no depth below min_score.
//
// One launch, one lane per pixel, a block per 32 x 8 tile:
//   * the main image's tile with its halo of r goes through LDS (each byte is
//     read by N windows x n witnesses); the halo is filled with the clamped
//     coordinates' bytes, so a window read needs no clamp of its own;
//   * the witnesses are walked in a run-time loop (their arguments are
//     wave-uniform: scalar loads), the sample arithmetic is warp_kernel's
//     (sgm.hip) restated, since that kernel keeps its instruction stream;
//   * a pixel's scores stay in registers: best[NW] is kept sorted, largest
//     first, by one pass of compare-and-swap per defined witness -- every index
//     is a compile-time one, so the array is registers for every NW (the code
//     object's .private_segment_fixed_size is 0 for all 16) -- and the mean adds
//     its first k' entries in that order;
//   * integer sums in 32 bits; double only for the one division per (pixel,
//     witness) and the mean.
#include "sgm_internal.h"

namespace smvs_hip {

constexpr int PH_TILE_W = 32, PH_TILE_H = 8;      // pixels per block
constexpr int PH_MAX_R = 3;
constexpr int PH_LDS_W = PH_TILE_W + 2 * PH_MAX_R;
constexpr int PH_LDS_H = PH_TILE_H + 2 * PH_MAX_R;
constexpr int PH_PITCH = PH_LDS_W + 2;            // 40 bytes: whole dwords per row

struct PhotoArgs {
    const uint8_t *main_img;
    const float *depth;
    float *out, *confidence;    // confidence, views: null when not asked for
    uint8_t *views;
    int w, h, n, radius, best_k, min_views;
    float min_score;
    SgmPhotoWitness wit[SMVS_MAX_SUBS];
};
static_assert(sizeof(PhotoArgs) <= 4096, "kernel arguments: 4 KB at the most");

// warped_neighbors_for_depth (sgm_stereo.cc:163-188) for main pixel (xc, yc) at
// `depth`, operation for operation as warp_kernel evaluates it; *inside stated
// positively (a coordinate that is not a number is outside).
__device__ __forceinline__ int
photo_sample(SgmPhotoWitness const &W, int xc, int yc, float depth, bool *inside)
{
#pragma clang fp contract(off)
    float const px = 0.5f + (float)xc, py = 0.5f + (float)yc;
    float tp[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        float s = 0.0f;
        s += W.M[3 * r + 0] * px;
        s += W.M[3 * r + 1] * py;
        s += W.M[3 * r + 2] * 1.f;
        tp[r] = s;
    }
    float const xmax = (float)(W.nw - 1), ymax = (float)(W.nh - 1);
    float p0 = tp[0] * depth + W.t[0];
    float p1 = tp[1] * depth + W.t[1];
    float const p2 = tp[2] * depth + W.t[2];
    p0 /= p2;
    p1 /= p2;
    p0 -= 0.5f;
    p1 -= 0.5f;
    *inside = !(p2 < 0) && p0 >= 0 && p1 >= 0 && p0 <= xmax && p1 <= ymax;
    if (!*inside)
        return 0;
    // mve::Image<uint8_t>::linear_at [MVE-unverified]
    float const fx = fmaxf(0.0f, fminf(xmax, p0));
    float const fy = fmaxf(0.0f, fminf(ymax, p1));
    int const ix = (int)fx, iy = (int)fy;
    int const ix1 = min(ix + 1, W.nw - 1), iy1 = min(iy + 1, W.nh - 1);
    float const w1 = fx - (float)ix, w0 = 1.0f - w1;
    float const w3 = fy - (float)iy, w2 = 1.0f - w3;
    const uint8_t *r0 = W.image + (size_t)iy * W.nw;
    const uint8_t *r1 = W.image + (size_t)iy1 * W.nw;
    float const v1 = (float)r0[ix];
    float const v2 = (float)r0[ix1];
    float const v3 = (float)r1[ix];
    float const v4 = (float)r1[ix1];
    return (int)(uint8_t)(v1 * (w0 * w2) + v2 * (w1 * w2) + v3 * (w0 * w3) + v4 * (w1 * w3)
        + 0.5f);
}

// NW: the size of the sorted score list, at least A.n.
template <int NW>
__global__ void __launch_bounds__(PH_TILE_W * PH_TILE_H)
sgm_photo_kernel(PhotoArgs A)
{
#pragma clang fp contract(off)
    __shared__ uint8_t tile[PH_LDS_H * PH_PITCH];
    int const r = A.radius;
    int const tx = (int)threadIdx.x, ty = (int)threadIdx.y;
    int const x0 = (int)blockIdx.x * PH_TILE_W, y0 = (int)blockIdx.y * PH_TILE_H;
    int const lw = PH_TILE_W + 2 * r, lh = PH_TILE_H + 2 * r;
    for (int idx = ty * PH_TILE_W + tx; idx < lw * lh; idx += PH_TILE_W * PH_TILE_H) {
        int const ly = idx / lw, lx = idx - ly * lw;
        int const gx = min(max(x0 - r + lx, 0), A.w - 1);
        int const gy = min(max(y0 - r + ly, 0), A.h - 1);
        tile[ly * PH_PITCH + lx] = A.main_img[(size_t)gy * A.w + gx];
    }
    __syncthreads();
    int const x = x0 + tx, y = y0 + ty;
    if (x >= A.w || y >= A.h)
        return;
    size_t const o = (size_t)y * A.w + x;
    float const a = A.depth[o];
    float conf = -1.0f;
    int c = 0;
    if (a > 0.0f) {
        int const nwin = (2 * r + 1) * (2 * r + 1);
        double best[NW];
#pragma unroll
        for (int s = 0; s < NW; ++s)
            best[s] = -2.0;
        for (int k = 0; k < A.n; ++k) {
            SgmPhotoWitness const &W = A.wit[k];
            int SA = 0, SB = 0, SAB = 0, SAA = 0, SBB = 0;
            bool defined = true;
            for (int j = -r; j <= r && defined; ++j) {
                int const yc = min(max(y + j, 0), A.h - 1);
                const uint8_t *row = tile + (ty + r + j) * PH_PITCH + tx + r;
                for (int i = -r; i <= r; ++i) {
                    int const xc = min(max(x + i, 0), A.w - 1);
                    bool inside;
                    int const vb = photo_sample(W, xc, yc, a, &inside);
                    int const va = (int)row[i];
                    defined = defined && inside;
                    SA += va;
                    SB += vb;
                    SAB += va * vb;
                    SAA += va * va;
                    SBB += vb * vb;
                }
            }
            if (!defined)
                continue;
            ++c;
            int const cov = nwin * SAB - SA * SB;
            int const va = nwin * SAA - SA * SA;
            int const vb = nwin * SBB - SB * SB;
            double score = 0.0;
            if (va != 0 && vb != 0) {
                // (both products are integers below 2^53: exact in double)
                double const num = (double)cov * (double)abs(cov);
                double const den = (double)va * (double)vb;
                score = num / den;
            }
            // into the sorted list: the larger of the two stays, the smaller moves on
#pragma unroll
            for (int s = 0; s < NW; ++s) {
                bool const up = score > best[s];
                double const t = best[s];
                best[s] = up ? score : t;
                score = up ? t : score;
            }
        }
        int const need = A.min_views > 1 ? A.min_views : 1;
        if (c >= need) {
            int const kk = min(A.best_k != 0 ? A.best_k : A.n, c);
            double sum = 0.0;
#pragma unroll
            for (int s = 0; s < NW; ++s)
                sum = s < kk ? sum + best[s] : sum;
            conf = (float)(sum / (double)kk);
        }
        A.out[o] = conf < A.min_score ? 0.0f : a;
    } else if (A.out != A.depth) {
        A.out[o] = a;       // (a pixel that is not valid keeps its bits)
    }
    if (A.confidence != nullptr)
        A.confidence[o] = conf;
    if (A.views != nullptr)
        A.views[o] = (uint8_t)c;
}

template <int NW>
static void
launch_photo_n(PhotoArgs const &A, dim3 grid, hipStream_t stream)
{
    if constexpr (NW > SMVS_MAX_SUBS)
        return;
    else if (A.n == NW)
        hipLaunchKernelGGL(sgm_photo_kernel<NW>, grid, dim3(PH_TILE_W, PH_TILE_H), 0, stream, A);
    else
        launch_photo_n<NW + 1>(A, grid, stream);
}

// (declared in sgm_internal.h)
int
check_sgm_photo(const smvs_sgm_photo_options *photo, int n)
{
    SMVS_REQUIRE(photo != nullptr, "null photo options (radius, best_k, min_views, min_score)");
    SMVS_REQUIRE(photo->radius >= 0 && photo->radius <= PH_MAX_R,
        "photo radius must be in [0, 3]");
    SMVS_REQUIRE(photo->best_k >= 0 && photo->best_k <= n,
        "photo best_k must be in [0, n_neighbors + n_witness]");
    SMVS_REQUIRE(photo->min_views >= 0 && photo->min_views <= n,
        "photo min_views must be in [0, n_neighbors + n_witness]");
    // (a NaN fails both comparisons)
    SMVS_REQUIRE(photo->min_score >= -1.0f && photo->min_score <= 1.0f,
        "photo min_score must be in [-1, 1]");
    return SMVS_OK;
}

// (declared in sgm_internal.h)
int
sgm_launch_photo(Workspace &ws, SgmProfile *prof, const uint8_t *d_main, int w, int h,
    const float *d_depth, const SgmPhotoWitness *witnesses, int n,
    smvs_sgm_photo_options const &opts, float *d_out, float *d_confidence, uint8_t *d_views)
{
    PhotoArgs A = { d_main, d_depth, d_out, d_confidence, d_views, w, h, n, opts.radius,
        opts.best_k, opts.min_views, opts.min_score, {} };
    for (int k = 0; k < SMVS_MAX_SUBS; ++k)
        A.wit[k] = witnesses[k < n ? k : 0];
    dim3 const grid((unsigned)((w + PH_TILE_W - 1) / PH_TILE_W),
        (unsigned)((h + PH_TILE_H - 1) / PH_TILE_H));
    {
        SgmKernelTimer timer(prof, ws.stream, SMVS_SGM_K_MERGE);
        launch_photo_n<1>(A, grid, ws.stream);
    }
    SMVS_HIP_CHECK(hipGetLastError());
    return SMVS_OK;
}

} // namespace smvs_hip

using namespace smvs_hip;

// the kernel alone, on a map and images of the caller
extern "C" int
smvs_sgm_photo_check(int device, const uint8_t *main_img, int w, int h, const float *depth,
    const smvs_sgm_neighbor *witnesses, int n, const smvs_sgm_photo_options *opts, float *out,
    float *confidence, uint8_t *views)
{
    SMVS_REQUIRE(opts != nullptr, "null photo options (radius, best_k, min_views, min_score)");
    SMVS_REQUIRE(opts->radius >= 1 && opts->radius <= PH_MAX_R,
        "photo radius must be in [1, 3] (smvs_sgm_photo_check is the test itself)");
    SMVS_REQUIRE(n >= 1 && n <= SMVS_MAX_SUBS, "n must be in [1, SMVS_MAX_SUBS]");
    if (int const rc = check_sgm_photo(opts, n); rc != SMVS_OK)
        return rc;
    SMVS_REQUIRE(main_img && depth && witnesses && out, "null argument");
    SMVS_REQUIRE(w >= 1 && h >= 1 && (size_t)w * h < ((size_t)1 << 31), "bad map size");
    size_t at[SMVS_MAX_SUBS + 1] = { 0 };
    for (int k = 0; k < n; ++k) {
        SMVS_REQUIRE(witnesses[k].image && witnesses[k].width >= 1 && witnesses[k].height >= 1
                && (size_t)witnesses[k].width * witnesses[k].height < ((size_t)1 << 31),
            "bad witness image");
        at[k + 1] = at[k] + (size_t)witnesses[k].width * witnesses[k].height;
    }
    int rc;
    WorkspaceLease lease(device);
    if (lease.w == nullptr)
        return SMVS_ERR_HIP;
    Workspace &ws = *lease.w;
    SgmProfile prof;
    size_t const npix = (size_t)w * h;
    uint8_t *d_main = nullptr, *d_wit = nullptr, *d_views = nullptr;
    float *d_depth = nullptr, *d_conf = nullptr;
    // (confidence, then views, in one slot)
    if ((rc = ws.ensure(WS_MAIN, npix, &d_main)) || (rc = ws.ensure(WS_PHOTO, at[n], &d_wit))
        || (rc = ws.ensure(WS_FWD0, npix, &d_depth))
        || (rc = ws.ensure(WS_PHOTO_OUT, npix * (sizeof(float) + 1), &d_conf))
        || (rc = ws.upload(d_main, main_img, npix))
        || (rc = ws.upload(d_depth, depth, sizeof(float) * npix)))
        return rc;
    d_views = reinterpret_cast<uint8_t *>(d_conf + npix);
    SgmPhotoWitness W[SMVS_MAX_SUBS];
    for (int k = 0; k < n; ++k) {
        smvs_sgm_neighbor const &N = witnesses[k];
        if ((rc = ws.upload(d_wit + at[k], N.image, at[k + 1] - at[k])))
            return rc;
        W[k].image = d_wit + at[k];
        W[k].nw = N.width;
        W[k].nh = N.height;
        for (int i = 0; i < 9; ++i)
            W[k].M[i] = N.M_fwd[i];
        for (int i = 0; i < 3; ++i)
            W[k].t[i] = N.t_fwd[i];
    }
    if ((rc = sgm_launch_photo(ws, &prof, d_main, w, h, d_depth, W, n, *opts, d_depth,
             confidence != nullptr ? d_conf : nullptr, views != nullptr ? d_views : nullptr))
        || (rc = ws.download(out, d_depth, sizeof(float) * npix)))
        return rc;
    if (confidence != nullptr && (rc = ws.download(confidence, d_conf, sizeof(float) * npix)))
        return rc;
    if (views != nullptr && (rc = ws.download(views, d_views, npix)))
        return rc;
    SMVS_HIP_CHECK(hipStreamSynchronize(ws.stream));
    return SMVS_OK;
}
