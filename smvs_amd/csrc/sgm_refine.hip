// Multi-view plane refinement sweeps on a depth map on gfx950 (not in the
// reference; include/smvs_hip.h, "Multi-view plane refinement sweeps", has the
// definition): every pixel holds a plane hypothesis (depth a, slants gx, gy), its
// confidence is the photo test's with the window's samples at the plane's depths,
// and red-black half-sweeps let a pixel adopt a 4-neighbour's extrapolated plane
// or a hashed perturbation of its own whenever that raises the confidence.
//
// Launches: one start launch (a lane per pixel, 32 x 8 tile: the photo test's
// confidence of (a, 0, 0)), 2 x sweeps half-sweep launches on the state planes in
// place, one end launch (out, slant).  One kernel serves the start and the
// half-sweeps; all under timers of class SMVS_SGM_K_MERGE.
//   * A half-sweep has a lane per ACTIVE pixel: a block of 32 x 8 lanes serves a
//     tile of 64 x 8 pixels, lane (x', y) the pixel x = x0 + 2 x' + ((y + c + x0)
//     & 1), so every wave is full.  The four neighbours have the other colour and
//     no lane writes them in this launch: in place is race-free.
//   * The main image's tile with its halo of r goes through LDS as in
//     sgm_photo_kernel (clamped halo bytes); SA and SAA of the window are formed
//     once per pixel and launch, the candidates add SB, SAB, SBB only.
//   * The neighbours' hypotheses are read from the state planes in global memory
//     (four reads per lane and plane, two of them in the lane's own row).
//   * One device function, refine_confidence, evaluates a hypothesis; it has one
//     call site, in a run-time loop over the candidates (start: the one
//     candidate (a, 0, 0)), so the code is there once.  The sorted score list is
//     the photo kernel's: compile-time indices, registers for every NW (the code
//     object's .private_segment_fixed_size is 0 for all 16).
//   * refine_sample is photo_sample of sgm_photo.hip restated, as that file
//     restates warp_kernel: every kernel of the parent keeps its instruction
//     stream.
#include "sgm_internal.h"

namespace smvs_hip {

constexpr int RF_BLOCK_W = 32, RF_BLOCK_H = 8;    // lanes per block
constexpr int RF_MAX_R = 3;
constexpr int RF_TILE_W = 2 * RF_BLOCK_W;         // pixels per row of a half-sweep's tile
constexpr int RF_LDS_H = RF_BLOCK_H + 2 * RF_MAX_R;
constexpr int RF_PITCH = RF_TILE_W + 2 * RF_MAX_R + 2;    // 72 bytes: whole dwords per row

struct RefineArgs {
    const uint8_t *main_img;
    const float *depth;         // the input map (read by the start launch)
    float *a, *gx, *gy, *conf;  // the state planes
    uint8_t *views;
    int w, h, n, radius, best_k, min_views;
    int colour;                 // -1: the start launch; 0, 1: a half-sweep
    int t, samples, fill;
    float depth_step, slant_step, scale;    // scale: 2^-t
    uint32_t seed;
    SgmPhotoWitness wit[SMVS_MAX_SUBS];
};
static_assert(sizeof(RefineArgs) <= 4096, "kernel arguments: 4 KB at the most");

// photo_sample of sgm_photo.hip, operation for operation.
__device__ __forceinline__ int
refine_sample(SgmPhotoWitness const &W, int xc, int yc, float depth, bool *inside)
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

__device__ __forceinline__ uint32_t
refine_mix(uint32_t v)
{
    v ^= v >> 16;
    v *= 0x7feb352du;
    v ^= v >> 15;
    v *= 0x846ca68bu;
    v ^= v >> 16;
    return v;
}

// u_j of the definition: a multiple of 2^-23 in [-1, 1), exact
__device__ __forceinline__ float
refine_unit(uint32_t h0, uint32_t j)
{
    uint32_t const hj = refine_mix(h0 + j * 0x9e3779b9u);
    return (float)((int32_t)(hj >> 8) - 8388608) * 0x1p-23f;
}

// The confidence of the hypothesis (a, gx, gy) at (x, y): `centre` is the pixel's
// byte in the LDS tile, SA and SAA the sums of its window; *views: the number of
// defined witnesses.
template <int NW>
__device__ __forceinline__ float
refine_confidence(RefineArgs const &A, const uint8_t *centre, int x, int y, int SA, int SAA,
    float a, float gx, float gy, int *views)
{
#pragma clang fp contract(off)
    int const r = A.radius;
    int const nwin = (2 * r + 1) * (2 * r + 1);
    int const va = nwin * SAA - SA * SA;
    double best[NW];
#pragma unroll
    for (int s = 0; s < NW; ++s)
        best[s] = -2.0;
    int c = 0;
    for (int k = 0; k < A.n; ++k) {
        SgmPhotoWitness const &W = A.wit[k];
        int SB = 0, SAB = 0, SBB = 0;
        bool defined = true;
        for (int j = -r; j <= r && defined; ++j) {
            int const yc = min(max(y + j, 0), A.h - 1);
            const uint8_t *row = centre + j * RF_PITCH;
            for (int i = -r; i <= r; ++i) {
                int const xc = min(max(x + i, 0), A.w - 1);
                float d = a + gx * (float)i;
                d = d + gy * (float)j;
                bool inside = false;
                int vb = 0;
                if (d > 0.0f)
                    vb = refine_sample(W, xc, yc, d, &inside);
                int const v = (int)row[i];
                defined = defined && inside;
                SB += vb;
                SAB += v * vb;
                SBB += vb * vb;
            }
        }
        if (!defined)
            continue;
        ++c;
        int const cov = nwin * SAB - SA * SB;
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
    *views = c;
    int const need = A.min_views > 1 ? A.min_views : 1;
    if (c < need)
        return -1.0f;
    int const kk = min(A.best_k != 0 ? A.best_k : A.n, c);
    double sum = 0.0;
#pragma unroll
    for (int s = 0; s < NW; ++s)
        sum = s < kk ? sum + best[s] : sum;
    return (float)(sum / (double)kk);
}

// NW: the size of the sorted score list, at least A.n.
template <int NW>
__global__ void __launch_bounds__(RF_BLOCK_W * RF_BLOCK_H)
sgm_refine_kernel(RefineArgs A)
{
#pragma clang fp contract(off)
    __shared__ uint8_t tile[RF_LDS_H * RF_PITCH];
    int const r = A.radius;
    bool const start = A.colour < 0;
    int const tx = (int)threadIdx.x, ty = (int)threadIdx.y;
    int const tw = start ? RF_BLOCK_W : RF_TILE_W;
    int const x0 = (int)blockIdx.x * tw, y0 = (int)blockIdx.y * RF_BLOCK_H;
    int const lw = tw + 2 * r, lh = RF_BLOCK_H + 2 * r;
    for (int idx = ty * RF_BLOCK_W + tx; idx < lw * lh; idx += RF_BLOCK_W * RF_BLOCK_H) {
        int const ly = idx / lw, lx = idx - ly * lw;
        int const gx = min(max(x0 - r + lx, 0), A.w - 1);
        int const gy = min(max(y0 - r + ly, 0), A.h - 1);
        tile[ly * RF_PITCH + lx] = A.main_img[(size_t)gy * A.w + gx];
    }
    __syncthreads();
    int const y = y0 + ty;
    int const lx = start ? tx : 2 * tx + ((y + A.colour + x0) & 1);
    int const x = x0 + lx;
    if (x >= A.w || y >= A.h)
        return;
    size_t const o = (size_t)y * A.w + x;
    // the pixel's hypothesis: none is a = 0.0f (a hypothesis has a > 0)
    float ca = 0.0f, cgx = 0.0f, cgy = 0.0f, cconf = -1.0f, din = 0.0f;
    int cviews = 0;
    if (start) {
        din = A.depth[o];
    } else {
        ca = A.a[o];
        if (!(ca > 0.0f) && A.fill == 0)
            return;
        cgx = A.gx[o];
        cgy = A.gy[o];
        cconf = A.conf[o];
        cviews = (int)A.views[o];
    }
    bool has = ca > 0.0f, changed = start;
    const uint8_t *centre = tile + (ty + r) * RF_PITCH + lx + r;
    int SA = 0, SAA = 0;
    for (int j = -r; j <= r; ++j)
        for (int i = -r; i <= r; ++i) {
            int const v = (int)centre[j * RF_PITCH + i];
            SA += v;
            SAA += v * v;
        }
    uint32_t const site = (uint32_t)o;
    int const q0 = start ? -1 : 0, q1 = start ? 0 : 4 + A.samples;
    for (int q = q0; q < q1; ++q) {
        float na = 0.0f, ngx = 0.0f, ngy = 0.0f;
        bool ok;
        if (q < 0) {
            na = din;
            ok = din > 0.0f;
        } else if (q < 4) {
            // left, right, up, down: the neighbour's plane, extrapolated to here
            int const dx = q == 0 ? -1 : (q == 1 ? 1 : 0);
            int const dy = q == 2 ? -1 : (q == 3 ? 1 : 0);
            int const xn = x + dx, yn = y + dy;
            ok = xn >= 0 && xn < A.w && yn >= 0 && yn < A.h;
            if (ok) {
                size_t const on = (size_t)yn * A.w + xn;
                float const an = A.a[on];
                ngx = A.gx[on];
                ngy = A.gy[on];
                float const step = dy == 0 ? ngx : ngy;
                na = (dx + dy) < 0 ? an + step : an - step;
                ok = an > 0.0f && na > 0.0f;
            }
        } else {
            ok = has;
            if (ok) {
                uint32_t const m = (uint32_t)(q - 4);
                uint32_t const h0 = refine_mix(A.seed
                    ^ refine_mix(site ^ refine_mix((uint32_t)A.t * 16u + m)));
                float const u1 = refine_unit(h0, 1u), u2 = refine_unit(h0, 2u),
                            u3 = refine_unit(h0, 3u);
                float e = ca * A.depth_step;
                e = e * A.scale;
                na = ca + e * u1;
                float g = ca * A.slant_step;
                g = g * A.scale;
                ngx = cgx + g * u2;
                ngy = cgy + g * u3;
                ok = na > 0.0f;
            }
        }
        if (!ok)
            continue;
        int nviews;
        float const nconf = refine_confidence<NW>(A, centre, x, y, SA, SAA, na, ngx, ngy,
            &nviews);
        if (q < 0 || nconf > cconf) {
            ca = na;
            cgx = ngx;
            cgy = ngy;
            cconf = nconf;
            cviews = nviews;
            has = true;
            changed = true;
        }
    }
    if (!changed)
        return;
    A.a[o] = ca;
    A.gx[o] = cgx;
    A.gy[o] = cgy;
    A.conf[o] = cconf;
    A.views[o] = (uint8_t)cviews;
}

// The end rule: out and slant from the state planes.
__global__ void __launch_bounds__(256)
sgm_refine_end_kernel(const float *__restrict__ a, const float *__restrict__ gx,
    const float *__restrict__ gy, const float *__restrict__ conf, const float *depth, float *out,
    float *__restrict__ slant, float min_score, size_t npix)
{
    size_t const o = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= npix)
        return;
    float const v = a[o];
    if (v > 0.0f)
        out[o] = conf[o] < min_score ? 0.0f : v;
    else if (out != depth)
        out[o] = depth[o];      // (a pixel without a hypothesis keeps its bits)
    if (slant != nullptr) {
        slant[2 * o] = gx[o];
        slant[2 * o + 1] = gy[o];
    }
}

template <int NW>
static void
launch_refine_n(RefineArgs const &A, dim3 grid, hipStream_t stream)
{
    if constexpr (NW > SMVS_MAX_SUBS)
        return;
    else if (A.n == NW)
        hipLaunchKernelGGL(sgm_refine_kernel<NW>, grid, dim3(RF_BLOCK_W, RF_BLOCK_H), 0, stream,
            A);
    else
        launch_refine_n<NW + 1>(A, grid, stream);
}

// (declared in sgm_internal.h)
int
check_sgm_refine(const smvs_sgm_refine_options *refine)
{
    SMVS_REQUIRE(refine != nullptr,
        "null refine options (sweeps, samples, depth_step, slant_step, seed, fill)");
    SMVS_REQUIRE(refine->sweeps >= 0 && refine->sweeps <= 8, "refine sweeps must be in [0, 8]");
    SMVS_REQUIRE(refine->samples >= 0 && refine->samples <= 8,
        "refine samples must be in [0, 8]");
    // (a NaN fails both comparisons)
    SMVS_REQUIRE(refine->depth_step >= 0.0f && refine->depth_step <= 1.0f,
        "refine depth_step must be in [0, 1]");
    SMVS_REQUIRE(refine->slant_step >= 0.0f && refine->slant_step <= 1.0f,
        "refine slant_step must be in [0, 1]");
    SMVS_REQUIRE(refine->fill == 0 || refine->fill == 1, "refine fill must be 0 or 1");
    return SMVS_OK;
}

// (declared in sgm_internal.h)
int
sgm_launch_refine(Workspace &ws, SgmProfile *prof, const uint8_t *d_main, int w, int h,
    const float *d_depth, const SgmPhotoWitness *witnesses, int n,
    smvs_sgm_photo_options const &photo, smvs_sgm_refine_options const &refine, float *d_state,
    float *d_out, float *d_slant, float *d_confidence, uint8_t *d_views)
{
    size_t const npix = (size_t)w * h;
    RefineArgs A = { d_main, d_depth, d_state, d_state + npix, d_state + 2 * npix, d_confidence,
        d_views, w, h, n, photo.radius, photo.best_k, photo.min_views, -1, 0, refine.samples,
        refine.fill, refine.depth_step, refine.slant_step, 1.0f, refine.seed, {} };
    for (int k = 0; k < SMVS_MAX_SUBS; ++k)
        A.wit[k] = witnesses[k < n ? k : 0];
    unsigned const rows = (unsigned)((h + RF_BLOCK_H - 1) / RF_BLOCK_H);
    {
        SgmKernelTimer timer(prof, ws.stream, SMVS_SGM_K_MERGE);
        launch_refine_n<1>(A, dim3((unsigned)((w + RF_BLOCK_W - 1) / RF_BLOCK_W), rows),
            ws.stream);
    }
    SMVS_HIP_CHECK(hipGetLastError());
    dim3 const half((unsigned)((w + RF_TILE_W - 1) / RF_TILE_W), rows);
    for (int t = 0; t < refine.sweeps; ++t) {
        A.t = t;
        A.scale = 1.0f / (float)(1 << t);       // 2^-t, exact
        for (int c = 0; c < 2; ++c) {
            A.colour = c;
            {
                SgmKernelTimer timer(prof, ws.stream, SMVS_SGM_K_MERGE);
                launch_refine_n<1>(A, half, ws.stream);
            }
            SMVS_HIP_CHECK(hipGetLastError());
        }
    }
    {
        SgmKernelTimer timer(prof, ws.stream, SMVS_SGM_K_MERGE);
        hipLaunchKernelGGL(sgm_refine_end_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256),
            0, ws.stream, A.a, A.gx, A.gy, A.conf, d_depth, d_out, d_slant, photo.min_score,
            npix);
    }
    SMVS_HIP_CHECK(hipGetLastError());
    return SMVS_OK;
}

} // namespace smvs_hip

using namespace smvs_hip;

// the kernels alone, on a map and images of the caller
extern "C" int
smvs_sgm_plane_refine(int device, const uint8_t *main_img, int w, int h, const float *depth,
    const smvs_sgm_neighbor *witnesses, int n, const smvs_sgm_photo_options *photo,
    const smvs_sgm_refine_options *refine, float *out, float *slant, float *confidence,
    uint8_t *views)
{
    SMVS_REQUIRE(photo != nullptr, "null photo options (radius, best_k, min_views, min_score)");
    SMVS_REQUIRE(photo->radius >= 1 && photo->radius <= RF_MAX_R,
        "photo radius must be in [1, 3] (smvs_sgm_plane_refine is the refinement itself)");
    SMVS_REQUIRE(n >= 1 && n <= SMVS_MAX_SUBS, "n must be in [1, SMVS_MAX_SUBS]");
    int rc;
    if ((rc = check_sgm_photo(photo, n)) != SMVS_OK || (rc = check_sgm_refine(refine)) != SMVS_OK)
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
    WorkspaceLease lease(device);
    if (lease.w == nullptr)
        return SMVS_ERR_HIP;
    Workspace &ws = *lease.w;
    SgmProfile prof;
    size_t const npix = (size_t)w * h;
    uint8_t *d_main = nullptr, *d_wit = nullptr, *d_views = nullptr;
    float *d_depth = nullptr, *d_conf = nullptr, *d_state = nullptr;
    // (confidence, then views, in one slot; a, gx, gy, then the slants, in another)
    if ((rc = ws.ensure(WS_MAIN, npix, &d_main)) || (rc = ws.ensure(WS_PHOTO, at[n], &d_wit))
        || (rc = ws.ensure(WS_FWD0, npix, &d_depth))
        || (rc = ws.ensure(WS_PHOTO_OUT, npix * (sizeof(float) + 1), &d_conf))
        || (rc = ws.ensure(WS_REFINE, npix * SGM_REFINE_PLANES, &d_state))
        || (rc = ws.upload(d_main, main_img, npix))
        || (rc = ws.upload(d_depth, depth, sizeof(float) * npix)))
        return rc;
    d_views = reinterpret_cast<uint8_t *>(d_conf + npix);
    float *const d_slant = d_state + 3 * npix;
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
    if ((rc = sgm_launch_refine(ws, &prof, d_main, w, h, d_depth, W, n, *photo, *refine, d_state,
             d_depth, slant != nullptr ? d_slant : nullptr, d_conf, d_views))
        || (rc = ws.download(out, d_depth, sizeof(float) * npix)))
        return rc;
    if (slant != nullptr && (rc = ws.download(slant, d_slant, 2 * sizeof(float) * npix)))
        return rc;
    if (confidence != nullptr && (rc = ws.download(confidence, d_conf, sizeof(float) * npix)))
        return rc;
    if (views != nullptr && (rc = ws.download(views, d_views, npix)))
        return rc;
    SMVS_HIP_CHECK(hipStreamSynchronize(ws.stream));
    return SMVS_OK;
}
