// Read off the surface: the depth and normal maps (Surface::get_depth_map /
// get_normal_map, reference: lib/surface.cc:155-183) and the lighting normal
// equations over the normal map (the accumulation loop of
// LightOptimizer::fit_lighting_to_image, lib/light_optimizer.cc:32-49).
#include "common.h"
#include "patch_bicubic.h"

namespace smvs_hip {

// depth / normal maps
struct MapArgs {
    const double *nodes;
    const uint8_t *patch_valid;
    const double *hermite_tab;
    float *depth;     // [H][W] or nullptr
    float *normals;   // [H][W][3] or nullptr
    int W, H, npx, stride, ps, start_x, start_y, num_patches;
    double inv_flen;
    int to_mve;          // depth in MVE's ray-length convention
    float invproj[9];    // CameraInfo::fill_inverse_calibration (to_mve)
};

__global__ void __launch_bounds__(256)
surface_maps_kernel(MapArgs A)
{
    int const pp = A.ps * A.ps;
    long long const gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    int const patch = (int)(gid / pp);
    int const pid = (int)(gid - (long long)patch * pp);
    if (patch >= A.num_patches || !A.patch_valid[patch])
        return;
    int const ix = patch % A.npx, iy = patch / A.npx;
    int const n00 = iy * A.stride + ix;
    int const ids[4] = { n00, n00 + 1, n00 + A.stride, n00 + A.stride + 1 };
    double th[16];
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int k = 0; k < 4; ++k)
            th[4 * n + k] = A.nodes[4 * (size_t)ids[n] + k];
    int const ci = pid % A.ps, cj = pid / A.ps;
    double w, wx, wy;
    eval_patch(A.hermite_tab, ci, cj, th, &w, &wx, &wy);
    int const px = A.start_x + ix * A.ps + ci;
    int const py = A.start_y + iy * A.ps + cj;
    size_t const o = (size_t)py * A.W + px;
    if (A.depth != nullptr) {
        float d = (float)w;
        if (A.to_mve) {
#pragma clang fp contract(off)
            // StereoView::write_depth_to_view (stereo_view.h:100-119):
            // mve::image::depthmap_convert_conventions, z-depth -> ray length
            // (`double len = px.norm(); dm *= len`, tests/golden/README.md M10;
            // the float operations of host/stereo_view.cc, the inverse of
            // mesh_cut.hip's mesh_prepare_kernel)
            float const fx = (float)px + 0.5f, fy = (float)py + 0.5f;
            float v[3];
#pragma unroll
            for (int r = 0; r < 3; ++r)
                v[r] = A.invproj[3 * r] * fx + A.invproj[3 * r + 1] * fy
                    + A.invproj[3 * r + 2];
            float const len = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
            d = (float)((double)d * (double)len);
        }
        A.depth[o] = d;
    }
    if (A.normals != nullptr) {
        // surface_derivative.cc:17-28
        double const x = (double)px + 0.5 - (double)A.W / 2.0;
        double const y = (double)py + 0.5 - (double)A.H / 2.0;
        double const nz = (x * wx + y * wy + w) * A.inv_flen;
        double const len = sqrt(wx * wx + wy * wy + nz * nz);
        A.normals[3 * o + 0] = (float)(wx / len);
        A.normals[3 * o + 1] = (float)(-wy / len);
        A.normals[3 * o + 2] = (float)(nz / len);
    }
}

static int
launch_maps(smvs_ctx *ctx, float *depth_dev, float *normals_dev,
    const float *inv_calibration9)
{
    MapArgs A;
    A.to_mve = inv_calibration9 != nullptr ? 1 : 0;
    for (int i = 0; i < 9; ++i)
        A.invproj[i] = inv_calibration9 != nullptr ? inv_calibration9[i] : 0.0f;
    A.nodes = ctx->nodes;
    A.patch_valid = ctx->patch_valid;
    A.hermite_tab = ctx->hermite_tab;
    A.depth = depth_dev;
    A.normals = normals_dev;
    A.W = ctx->width;
    A.H = ctx->height;
    A.npx = ctx->npx;
    A.stride = ctx->node_stride;
    A.ps = ctx->patchsize;
    A.start_x = ctx->start_x;
    A.start_y = ctx->start_y;
    A.num_patches = ctx->num_patches;
    A.inv_flen = (double)ctx->inv_flen;
    long long const items = (long long)ctx->num_patches * ctx->patchsize
        * ctx->patchsize;
    ScopedKernelTimer timer(ctx, SMVS_K_MISC);
    hipLaunchKernelGGL(surface_maps_kernel, dim3((unsigned)((items + 255) / 256)),
        dim3(256), 0, ctx->stream, A);
    SMVS_HIP_CHECK(hipGetLastError());
    return SMVS_OK;
}

// lighting normal equations: A += sh sh^T, b += sh I over valid pixels
__device__ __forceinline__ void
sh_basis_4_band(const double n[3], double sh[16])
{
    double const nx = n[0], ny = n[1], nz = n[2];
    double const x2 = nx * nx, y2 = ny * ny, z2 = nz * nz;
    sh[0] = 1.0; sh[1] = ny; sh[2] = nz; sh[3] = nx;
    sh[4] = nx * ny; sh[5] = ny * nz; sh[6] = -x2 - y2 + 2.0 * z2;
    sh[7] = nx * nz; sh[8] = x2 - y2;
    sh[9] = (3.0 * x2 - y2) * ny; sh[10] = nx * ny * nz;
    sh[11] = (4.0 * z2 - x2 - y2) * ny;
    sh[12] = (2.0 * z2 - 3.0 * x2 - 3.0 * y2) * nz;
    sh[13] = (4.0 * z2 - x2 - y2) * nx;
    sh[14] = (x2 - y2) * nz; sh[15] = (x2 - 3.0 * y2) * nx;
}

constexpr int LIGHT_BLOCKS = 512;

// partial[block][152]: upper triangle of A (136) then b (16)
__global__ void __launch_bounds__(256)
light_accumulate_kernel(const float *__restrict__ normals,
    const float *__restrict__ image, size_t num_pixels,
    double *__restrict__ partial)
{
    double acc[152];
#pragma unroll
    for (int i = 0; i < 152; ++i)
        acc[i] = 0.0;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
         p < num_pixels; p += (size_t)gridDim.x * blockDim.x) {
        double const n[3] = { (double)normals[3 * p], (double)normals[3 * p + 1],
            (double)normals[3 * p + 2] };
        double const len = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        float const iv = image[p];
        if (fabs(len - 1.0) > 1e-6 || iv < 0.05f)
            continue;
        double sh[16];
        sh_basis_4_band(n, sh);
        int k = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i)
#pragma unroll
            for (int j = i; j < 16; ++j)
                acc[k++] += sh[i] * sh[j];
#pragma unroll
        for (int i = 0; i < 16; ++i)
            acc[136 + i] += sh[i] * (double)iv;
    }
    __shared__ double red[4][152];
    int const lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < 152; ++i) {
        double s = acc[i];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1)
            s += __shfl_xor(s, off);
        if (lane == 0)
            red[wave][i] = s;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 152; i += blockDim.x)
        partial[(size_t)blockIdx.x * 152 + i] = red[0][i] + red[1][i]
            + red[2][i] + red[3][i];
}

__global__ void
light_finalize_kernel(const double *__restrict__ partial, int blocks,
    double *__restrict__ Ab)
{
    int const i = threadIdx.x;
    if (i >= 152)
        return;
    double s = 0.0;
    for (int b = 0; b < blocks; ++b)
        s += partial[(size_t)b * 152 + i];
    if (i >= 136) {
        Ab[256 + (i - 136)] = s;
        return;
    }
    // unpack upper-triangle index
    int r = 0, k = i;
    while (k >= 16 - r) {
        k -= 16 - r;
        r += 1;
    }
    int const c = r + k;
    Ab[r * 16 + c] = s;
    Ab[c * 16 + r] = s;
}

} // namespace smvs_hip

using namespace smvs_hip;

// Output scratch owned by the context (no allocation per call); it only grows.
static int
ensure_map_scratch(smvs_ctx *ctx, size_t floats)
{
    return device_grow(&ctx->map_scratch, &ctx->map_scratch_floats, floats);
}

// The maps asked for into the context's scratch, cleared first: the normals
// (3 floats per pixel) at its start, the depth behind them -- at its start
// when alone.  Never less room than a normal map's, which every caller but
// smvs_get_maps makes do with.  inv_calibration9: depth in MVE's convention.
static int
maps_to_scratch(smvs_ctx *ctx, bool depth, bool normals, const float *inv_calibration9)
{
    size_t const npix = (size_t)ctx->width * ctx->height;
    size_t const used = npix * ((normals ? 3 : 0) + (depth ? 1 : 0));
    int const rc = ensure_map_scratch(ctx, used > npix * 3 ? used : npix * 3);
    if (rc != SMVS_OK)
        return rc;
    float *buf = ctx->map_scratch;
    SMVS_HIP_CHECK(hipMemsetAsync(buf, 0, used * sizeof(float), ctx->stream));
    return launch_maps(ctx, depth ? buf + (normals ? npix * 3 : 0) : nullptr,
        normals ? buf : nullptr, inv_calibration9);
}

// ... and from there to the host (a null pointer: not this map); both maps
// into page-locked buffers without the staging copy.  `who` for the message.
static int
download_maps(smvs_ctx *ctx, const char *who, float *depth, float *normals,
    const float *inv_calibration9)
{
    if (!ctx->has_surface) {
        set_error("%s: no surface", who);
        return SMVS_ERR_STATE;
    }
    SMVS_HIP_CHECK(set_device(ctx->device));
    size_t const npix = (size_t)ctx->width * ctx->height;
    int rc = maps_to_scratch(ctx, depth != nullptr, normals != nullptr, inv_calibration9);
    if (rc != SMVS_OK)
        return rc;
    const float *nbuf = ctx->map_scratch;
    const float *dbuf = nbuf + (normals != nullptr ? npix * 3 : 0);
    if (depth != nullptr && normals != nullptr && host_pointer_is_pinned(depth)
        && host_pointer_is_pinned(normals)) {
        SMVS_HIP_CHECK(hipMemcpyAsync(depth, dbuf, npix * sizeof(float),
            hipMemcpyDeviceToHost, ctx->stream));
        SMVS_HIP_CHECK(hipMemcpyAsync(normals, nbuf, npix * 3 * sizeof(float),
            hipMemcpyDeviceToHost, ctx->stream));
        SMVS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        return SMVS_OK;
    }
    if (depth != nullptr
        && (rc = ctx_download(ctx, depth, dbuf, npix * sizeof(float))) != SMVS_OK)
        return rc;
    return normals == nullptr ? SMVS_OK
        : ctx_download(ctx, normals, nbuf, npix * 3 * sizeof(float));
}

extern "C" int
smvs_get_depth_map(smvs_ctx *ctx, float *depth)
{
    SMVS_REQUIRE(ctx && depth, "null argument");
    return download_maps(ctx, __func__, depth, nullptr, nullptr);
}

extern "C" int
smvs_get_normal_map(smvs_ctx *ctx, float *normals)
{
    SMVS_REQUIRE(ctx && normals, "null argument");
    return download_maps(ctx, __func__, nullptr, normals, nullptr);
}

extern "C" int
smvs_get_maps(smvs_ctx *ctx, const float *inv_calibration9, float *depth, float *normals)
{
    SMVS_REQUIRE(ctx != nullptr, "null context");
    SMVS_REQUIRE(depth != nullptr && normals != nullptr, "null output");
    return download_maps(ctx, __func__, depth, normals, inv_calibration9);
}

extern "C" int
smvs_light_accumulate_dev(smvs_ctx *ctx, double **Ab272_dev)
{
    SMVS_REQUIRE(ctx != nullptr, "null context");
    if (!ctx->has_surface || !ctx->has_shading) {
        set_error("smvs_light_accumulate: needs a surface and a shading image");
        return SMVS_ERR_STATE;
    }
    SMVS_HIP_CHECK(set_device(ctx->device));
    int rc;
    if (ctx->light_partial == nullptr
        && (rc = device_alloc(&ctx->light_partial,
                (size_t)LIGHT_BLOCKS * 152)) != SMVS_OK)
        return rc;
    if ((rc = maps_to_scratch(ctx, false, true, nullptr)) != SMVS_OK)
        return rc;
    double *partial = ctx->light_partial;
    hipError_t e;
    {
        ScopedKernelTimer timer(ctx, SMVS_K_MISC);
        hipLaunchKernelGGL(light_accumulate_kernel, dim3(LIGHT_BLOCKS),
            dim3(256), 0, ctx->stream, ctx->map_scratch, ctx->main_shading,
            (size_t)ctx->width * ctx->height, partial);
        hipLaunchKernelGGL(light_finalize_kernel, dim3(1), dim3(256), 0,
            ctx->stream, partial, LIGHT_BLOCKS, ctx->lightAb);
        e = hipGetLastError();
    }
    if (e == hipSuccess)
        e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        set_error("smvs_light_accumulate: %s", hipGetErrorString(e));
        return SMVS_ERR_HIP;
    }
    if (Ab272_dev != nullptr)
        *Ab272_dev = ctx->lightAb;
    return SMVS_OK;
}

extern "C" int
smvs_light_accumulate(smvs_ctx *ctx, double *A256, double *b16)
{
    SMVS_REQUIRE(ctx && A256 && b16, "null argument");
    int const rc = smvs_light_accumulate_dev(ctx, nullptr);
    return rc != SMVS_OK ? rc : smvs_light_download(ctx, A256, b16);
}

extern "C" int
smvs_light_upload(smvs_ctx *ctx, const double *A256, const double *b16)
{
    SMVS_REQUIRE(ctx && A256 && b16, "null argument");
    SMVS_HIP_CHECK(set_device(ctx->device));
    double host[272];
    memcpy(host, A256, 256 * sizeof(double));
    memcpy(host + 256, b16, 16 * sizeof(double));
    SMVS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    SMVS_HIP_CHECK(hipMemcpy(ctx->lightAb, host, sizeof(host), hipMemcpyHostToDevice));
    return SMVS_OK;
}

extern "C" int
smvs_light_download(smvs_ctx *ctx, double *A256, double *b16)
{
    SMVS_REQUIRE(ctx && A256 && b16, "null argument");
    SMVS_HIP_CHECK(set_device(ctx->device));
    double host[272];
    SMVS_HIP_CHECK(hipMemcpy(host, ctx->lightAb, sizeof(host),
        hipMemcpyDeviceToHost));
    memcpy(A256, host, 256 * sizeof(double));
    memcpy(b16, host + 256, 16 * sizeof(double));
    return SMVS_OK;
}
