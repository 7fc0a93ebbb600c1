// The joint bilateral upsample of the SGM depth map on gfx950:
// DepthOptimizer::depthmap_bilateral_filter (reference:
// lib/depth_optimizer.cc:957-1004), stand-alone on a pooled workspace
// (smvs_bilateral_upsample) and inside a view's context, guided by the main
// image the context holds (smvs_ctx_sgm_init_depth[_mve]).
#include "sgm_internal.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <mutex>

namespace smvs_hip {

// depth_optimizer.cc:957-1004
struct BilateralArgs {
    const float *dm;
    const float *ci;
    float *out;
    int dm_w, dm_h, w, h, channels, kernel_size;
    float sigma;
};

__device__ __forceinline__ float
exp_rounded(float x)
{
    return (float)exp((double)x);
}

__global__ void __launch_bounds__(256)
bilateral_kernel(BilateralArgs A)
{
#pragma clang fp contract(off)
    int const x = blockIdx.x * blockDim.x + threadIdx.x;
    int const y = blockIdx.y;
    if (x >= A.w)
        return;
    float const scale_x = (float)A.dm_w / (float)A.w;
    float const scale_y = (float)A.dm_h / (float)A.h;
    float acc_v = 0.0f, acc_w = 0.0f;
    for (int ky = -A.kernel_size; ky <= A.kernel_size; ++ky)
        for (int kx = -A.kernel_size; kx <= A.kernel_size; ++kx) {
            int const ci_x = min(max(x + kx, 0), A.w - 1);
            int const ci_y = min(max(y + ky, 0), A.h - 1);
            float fx = scale_x * (float)ci_x, fy = scale_y * (float)ci_y;
            fx = fminf(fmaxf(fx, 0.f), (float)A.dm_w - 1.f);
            fy = fminf(fmaxf(fy, 0.f), (float)A.dm_h - 1.f);
            int const dm_x = (int)fx, dm_y = (int)fy;
            float const dv = A.dm[(size_t)dm_y * A.dm_w + dm_x];
            if (dv == 0.0f)
                continue;
            // math::gaussian / gaussian_2d are std::exp on floats.  The
            // exponential is taken in double and rounded once: the correctly
            // rounded value, which the device's float expf does not give --
            // and which the host's (glibc) expf misses by an ulp in ~0.3 % of
            // its arguments (see bilateral_table_kernel).  So this path is
            // NOT the CPU path bit for bit: on the cases of
            // tests/test_gpu_bilateral.py the filtered map differs from it in
            // 8 of 394,616 pixels, by at most two ulps
            // (profiles/bilateral_forms_parity.txt; the tests allow 1e-5 of
            // the largest depth).  The forms with the host's tables are.
            float weight = 1.0f;
            weight *= exp_rounded(-((float)kx * (float)kx
                / (2.0f * A.sigma * A.sigma)
                + (float)ky * (float)ky / (2.0f * A.sigma * A.sigma)));
            for (int c = 0; c < A.channels; ++c) {
                float const diff =
                    A.ci[((size_t)ci_y * A.w + ci_x) * A.channels + c]
                    - A.ci[((size_t)y * A.w + x) * A.channels + c];
                weight *= exp_rounded(-(diff * diff) / (2.0f * 0.1f * 0.1f));
            }
            acc_v += dv * weight;
            acc_w += weight;
        }
    A.out[(size_t)y * A.w + x] = acc_w > 0 ? acc_v / acc_w : 0.0f;
}

// The same filter when the guidance image is a byte image divided by 255 (the
// main image a context holds): the colour weight of a tap is a function of the
// two bytes only.  The HOST evaluates the reference's own float expression
// with expf for all 256 x 256 pairs (math::gaussian is std::exp on floats, and
// glibc's expf is not correctly rounded in ~0.3 % of its arguments, so only the
// host's own values give the CPU path's weights bit for bit) and compresses
// them for LDS: the weight depends on the pair almost only through the
// difference d = tap - centre -- the float rounding of the two quotients
// leaves at most four distinct values per d -- so the table is 511 x 4 floats
// plus a 2-bit selector per pair: 24 KB.  No exponential on the device; the
// spatial weights of the (2 k + 1)^2 taps are kernel arguments.
constexpr int BIL_MAX_K = 7;
constexpr int BIL_VALS = 2048;            // 511 differences x 4 candidates (floats)
constexpr int BIL_SEL = 65536 / 16;       // 2-bit selectors, 16 per word
constexpr int BIL_TABLE_WORDS = BIL_VALS + BIL_SEL;
struct BilateralSpatial { float w[(2 * BIL_MAX_K + 1) * (2 * BIL_MAX_K + 1)]; };

// f = (float)b / 255.0f is inverted exactly by rounding f * 255
__global__ void __launch_bounds__(256)
float_to_byte_kernel(const float *__restrict__ in, uint8_t *__restrict__ out, size_t n)
{
#pragma clang fp contract(off)
    size_t const i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        out[i] = (uint8_t)(in[i] * 255.0f + 0.5f);
}

template <int C>
__global__ void __launch_bounds__(256)
bilateral_table_kernel(BilateralArgs A, const uint8_t *__restrict__ ci8,
    const uint32_t *__restrict__ table, BilateralSpatial S)
{
#pragma clang fp contract(off)
    __shared__ uint32_t lds[BIL_TABLE_WORDS];
    for (int i = threadIdx.x; i < BIL_TABLE_WORDS; i += 256)
        lds[i] = table[i];
    __syncthreads();
    const float *vals = reinterpret_cast<const float *>(lds);
    const uint32_t *sel = lds + BIL_VALS;
    int const x = blockIdx.x * blockDim.x + threadIdx.x;
    int const y = blockIdx.y;
    if (x >= A.w)
        return;
    float const scale_x = (float)A.dm_w / (float)A.w;
    float const scale_y = (float)A.dm_h / (float)A.h;
    int const ks = A.kernel_size, kw = 2 * ks + 1;
    unsigned centre[C];
#pragma unroll
    for (int c = 0; c < C; ++c)
        centre[c] = ci8[((size_t)y * A.w + x) * C + c];
    float acc_v = 0.0f, acc_w = 0.0f;
    for (int ky = -ks; ky <= ks; ++ky) {
        int const ci_y = min(max(y + ky, 0), A.h - 1);
        float fy = scale_y * (float)ci_y;
        fy = fminf(fmaxf(fy, 0.f), (float)A.dm_h - 1.f);
        const float *dm_row = A.dm + (size_t)(int)fy * A.dm_w;
        const uint8_t *ci_row = ci8 + (size_t)ci_y * A.w * C;
        for (int kx = -ks; kx <= ks; ++kx) {
            int const ci_x = min(max(x + kx, 0), A.w - 1);
            float fx = scale_x * (float)ci_x;
            fx = fminf(fmaxf(fx, 0.f), (float)A.dm_w - 1.f);
            float const dv = dm_row[(int)fx];
            if (dv == 0.0f)
                continue;
            float weight = 1.0f;
            weight *= S.w[(ky + ks) * kw + (kx + ks)];
#pragma unroll
            for (int c = 0; c < C; ++c) {
                unsigned const b = ci_row[ci_x * C + c];
                unsigned const pair = (centre[c] << 8) | b;
                unsigned const which = (sel[pair >> 4] >> ((pair & 15u) * 2u)) & 3u;
                weight *= vals[((b + 255u - centre[c]) << 2) | which];
            }
            acc_v += dv * weight;
            acc_w += weight;
        }
    }
    A.out[(size_t)y * A.w + x] = acc_w > 0 ? acc_v / acc_w : 0.0f;
}

// The compressed colour-weight table, or nullptr when some difference has
// more than four distinct weights (another libm: the exponentials are then
// taken on the device as in bilateral_kernel).
static const uint32_t *
bilateral_colour_table(void)
{
#pragma clang fp contract(off)
    static std::vector<uint32_t> table;
    static bool usable = false;
    static std::once_flag once;
    std::call_once(once, []() {
        std::vector<uint32_t> t(BIL_TABLE_WORDS, 0u);
        int count[511] = { 0 };
        bool ok = true;
        for (int a = 0; a < 256 && ok; ++a)
            for (int b = 0; b < 256; ++b) {
                // gaussian(tap - centre, 0.1) as the reference evaluates it on floats
                float const diff = (float)b / 255.0f - (float)a / 255.0f;
                float const wgt = expf(-(diff * diff) / (2.0f * 0.1f * 0.1f));
                uint32_t bits;
                memcpy(&bits, &wgt, sizeof(bits));
                int const d = b + 255 - a;
                int k = 0;
                while (k < count[d] && t[(size_t)d * 4 + k] != bits)
                    k += 1;
                if (k == count[d]) {
                    if (k == 4) {
                        ok = false;
                        break;
                    }
                    t[(size_t)d * 4 + k] = bits;
                    count[d] += 1;
                }
                unsigned const pair = ((unsigned)a << 8) | (unsigned)b;
                t[BIL_VALS + (pair >> 4)] |= (uint32_t)k << ((pair & 15u) * 2u);
            }
        usable = ok;
        table.swap(t);
    });
    return usable ? table.data() : nullptr;
}

// Round 6: the same weights as ONE lookup per tap and channel.  The colour
// weight of a pair of bytes is symmetric to the bit -- (float)b / 255 - (float)a
// / 255 changes its sign exactly when the bytes change places, and the weight
// squares it -- so the table of all pairs is a triangle of 256 x 257 / 2 floats
// = 131,584 bytes: it fits the CU's 160 KB of LDS whole.  A persistent grid of
// one workgroup of 1,024 lanes per CU loads it once and walks over the image;
// per tap and channel: minimum, maximum, the triangle's index, one LDS read (the
// compressed table above: two dependent LDS reads and twelve vector
// instructions, and the kernel was bound by both).  Half width BIL_TRI_K (the
// reference's default, depth_optimizer.h:70-72) with the window's columns
// unrolled -- the clamped column of the guidance image and the column of the
// depth map a tap reads are formed once per pixel, not once per tap.  Same taps,
// same order, same products: the filtered map is array_equal with the oracle's
// (tests/test_gpu_front.py).  SMVS_BILATERAL=compressed: the kernel above.
constexpr int BIL_TRI_K = 5;
constexpr int BIL_TRI_FLOATS = 256 * 257 / 2;
constexpr int BIL_TRI_THREADS = 1024;

template <int C>
__global__ void __launch_bounds__(BIL_TRI_THREADS)
bilateral_triangle_kernel(BilateralArgs A, const uint8_t *__restrict__ ci8,
    const float *__restrict__ triangle, BilateralSpatial S)
{
#pragma clang fp contract(off)
    extern __shared__ float tri[];
    for (int i = threadIdx.x; i < BIL_TRI_FLOATS; i += BIL_TRI_THREADS)
        tri[i] = triangle[i];
    __syncthreads();
    constexpr int KS = BIL_TRI_K, KW = 2 * KS + 1;
    float const scale_x = (float)A.dm_w / (float)A.w;
    float const scale_y = (float)A.dm_h / (float)A.h;
    long long const npix = (long long)A.w * A.h;
    for (long long pix = (long long)blockIdx.x * BIL_TRI_THREADS + threadIdx.x; pix < npix;
        pix += (long long)gridDim.x * BIL_TRI_THREADS) {
        int const y = (int)(pix / A.w), x = (int)(pix - (long long)y * A.w);
        unsigned centre[C];
#pragma unroll
        for (int c = 0; c < C; ++c)
            centre[c] = ci8[(size_t)pix * C + c];
        // the columns of the window: byte offset in a row of the guidance image,
        // column of the depth map
        int col_ci[KW], col_dm[KW];
#pragma unroll
        for (int k = 0; k < KW; ++k) {
            int const ci_x = min(max(x + k - KS, 0), A.w - 1);
            float fx = scale_x * (float)ci_x;
            fx = fminf(fmaxf(fx, 0.f), (float)A.dm_w - 1.f);
            col_ci[k] = ci_x * C;
            col_dm[k] = (int)fx;
        }
        float acc_v = 0.0f, acc_w = 0.0f;
#pragma unroll 1
        for (int ky = -KS; ky <= KS; ++ky) {
            int const ci_y = min(max(y + ky, 0), A.h - 1);
            float fy = scale_y * (float)ci_y;
            fy = fminf(fmaxf(fy, 0.f), (float)A.dm_h - 1.f);
            const float *dm_row = A.dm + (size_t)(int)fy * A.dm_w;
            const uint8_t *ci_row = ci8 + (size_t)ci_y * A.w * C;
            const float *sw = S.w + (ky + KS) * KW;
            // every load of a window row is issued before the first is used, the
            // bytes of a tap without depth included (a tap was: depth -> branch ->
            // bytes -> table, three round trips in a row, eleven times per row)
            float dv[KW];
            unsigned bytes[KW][C];
#pragma unroll
            for (int k = 0; k < KW; ++k) {
                dv[k] = dm_row[col_dm[k]];
#pragma unroll
                for (int c = 0; c < C; ++c)
                    bytes[k][c] = ci_row[col_ci[k] + c];
            }
#pragma unroll
            for (int k = 0; k < KW; ++k) {
                float weight = 1.0f;
                weight *= sw[k];
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    unsigned const b = bytes[k][c];
                    unsigned const lo = min(b, centre[c]), hi = max(b, centre[c]);
                    // byte offset 4 (hi (hi + 1) / 2 + lo) = (2 hi) hi + 2 hi + 4 lo:
                    // a shift, a 24-bit multiply-add, a shift-add
                    unsigned const h2 = hi << 1;
                    unsigned t;
                    asm("v_mad_u32_u24 %0, %1, %2, %1" : "=v"(t) : "v"(h2), "v"(hi));
                    weight *= *reinterpret_cast<const float *>(
                        reinterpret_cast<const char *>(tri) + (t + (lo << 2)));
                }
                // a tap without depth is skipped by the reference: it adds +0 to
                // both sums here, which leaves them as they are to the bit (the
                // sums start at +0 and the weights are positive: never -0)
                acc_v += dv[k] * weight;
                acc_w += dv[k] == 0.0f ? 0.0f : weight;
            }
        }
        A.out[pix] = acc_w > 0 ? acc_v / acc_w : 0.0f;
    }
}

// The triangle of colour weights (index hi (hi + 1) / 2 + lo), or nullptr when
// some pair is not symmetric to the bit (it always is, see above; checked
// because the bits are the host libm's).
static const float *
bilateral_colour_triangle(void)
{
#pragma clang fp contract(off)
    static std::vector<float> table;
    static bool usable = false;
    static std::once_flag once;
    std::call_once(once, []() {
        std::vector<float> t((size_t)BIL_TRI_FLOATS, 0.0f);
        bool ok = true;
        for (int a = 0; a < 256 && ok; ++a)
            for (int b = 0; b < 256; ++b) {
                // gaussian(tap - centre, 0.1) as the reference evaluates it on floats
                float const diff = (float)b / 255.0f - (float)a / 255.0f;
                float const wgt = expf(-(diff * diff) / (2.0f * 0.1f * 0.1f));
                int const lo = a < b ? a : b, hi = a < b ? b : a;
                size_t const at = (size_t)hi * (size_t)(hi + 1) / 2 + (size_t)lo;
                if (a <= b) {
                    t[at] = wgt;
                } else {
                    // (a > b: the mirrored pair has been stored)
                    if (std::memcmp(&t[at], &wgt, sizeof(float)) != 0) {
                        ok = false;
                        break;
                    }
                }
            }
        usable = ok;
        table.swap(t);
    });
    return usable ? table.data() : nullptr;
}

} // namespace smvs_hip

using namespace smvs_hip;

extern "C" int
smvs_bilateral_upsample(int device, const float *dm, int dm_w, int dm_h,
    const float *ci, int w, int h, int channels, float sigma, int kernel_size,
    float *out)
{
    SMVS_REQUIRE(dm && ci && out, "null argument");
    SMVS_REQUIRE(dm_w > 0 && dm_h > 0 && w > 0 && h > 0 && channels > 0
        && kernel_size >= 0 && sigma > 0.f, "bad argument");
    WorkspaceLease lease(device);
    if (lease.w == nullptr)
        return SMVS_ERR_HIP;
    Workspace &ws = *lease.w;
    float *d_dm = nullptr, *d_ci = nullptr, *d_out = nullptr;
    int rc;
    size_t const n = (size_t)w * h;
    if ((rc = ws.ensure(WS_BIL_DM, (size_t)dm_w * dm_h, &d_dm))
        || (rc = ws.ensure(WS_BIL_CI, n * channels, &d_ci))
        || (rc = ws.ensure(WS_BIL_OUT, n, &d_out))
        || (rc = ws.upload(d_dm, dm, sizeof(float) * dm_w * dm_h))
        || (rc = ws.upload(d_ci, ci, sizeof(float) * n * channels)))
        return rc;
    BilateralArgs A;
    A.dm = d_dm;
    A.ci = d_ci;
    A.out = d_out;
    A.dm_w = dm_w;
    A.dm_h = dm_h;
    A.w = w;
    A.h = h;
    A.channels = channels;
    A.kernel_size = kernel_size;
    A.sigma = sigma;
    SgmProfile prof;
    {
        SgmKernelTimer timer(&prof, ws.stream, SMVS_SGM_K_BILATERAL);
        hipLaunchKernelGGL(bilateral_kernel, dim3((w + 255) / 256, h), dim3(256), 0,
            ws.stream, A);
    }
    SMVS_HIP_CHECK(hipGetLastError());
    return ws.download(out, d_out, sizeof(float) * n);
}

// The same filter for a view whose context already holds the main image
// (smvs_ctx_upload_image): guided by that image, and the full-size result
// stays on the device as the depth map the visibility tests of
// smvs_topology_subviews compare with (lib/depth_optimizer.cc:35-51 hands the
// filtered map to both).  Saves the upload of the float image (25 MB at
// 1920 x 1080 x 3) and of the result, once per topology pass.
// The low-resolution SGM map from page-locked host memory (read over the bus)
// to the device.  from_mve: the map is the view's "smvs-sgm" embedding as
// StereoView::write_depth_to_view stored it (MVE's ray-length convention) and is
// turned into z-depth on the way -- mve::image::depthmap_convert_conventions
// with the float operations of host/stereo_view.cc (StereoView::get_sgm_depth,
// stereo_view.h:121-135), so the same bits as the host conversion.
struct SgmMapUpload {
    const float *src;
    float *dst;
    int w, h;
    int from_mve;
    float invproj[9];
};

__global__ void __launch_bounds__(256)
sgm_map_upload_kernel(SgmMapUpload A)
{
#pragma clang fp contract(off)
    size_t const i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)A.w * A.h)
        return;
    float d = A.src[i];
    if (A.from_mve != 0) {
        int const y = (int)(i / (size_t)A.w), x = (int)(i - (size_t)y * A.w);
        float const px = (float)x + 0.5f, py = (float)y + 0.5f;
        float v[3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
            v[r] = A.invproj[3 * r] * px + A.invproj[3 * r + 1] * py + A.invproj[3 * r + 2];
        float const len = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        // `double len = px.norm(); dm *= 1.0 / len` [MVE-unverified, M10]
        double const len_d = (double)len;
        // (from_mve == 2: the map is still the z-depth the SGM front end produced;
        // the view would store it as ray length first -- write_depth_to_view,
        // `dm *= len` -- and the reference reads it back through that embedding)
        if (A.from_mve == 2)
            d = (float)((double)d * len_d);
        d = (float)((double)d * (1.0 / len_d));
    }
    A.dst[i] = d;
}

static int
sgm_init_depth(smvs_ctx *ctx, const float *dm, int dm_w, int dm_h, const float *inv_calibration9,
    int dm_is_z_depth, float sigma, int kernel_size, float *out);

extern "C" int
smvs_ctx_sgm_init_depth(smvs_ctx *ctx, const float *dm, int dm_w, int dm_h,
    float sigma, int kernel_size, float *out)
{
    return sgm_init_depth(ctx, dm, dm_w, dm_h, nullptr, 0, sigma, kernel_size, out);
}

extern "C" int
smvs_ctx_sgm_init_depth_mve(smvs_ctx *ctx, const float *dm, int dm_w, int dm_h,
    const float *inv_calibration9, int dm_is_z_depth, float sigma, int kernel_size, float *out)
{
    SMVS_REQUIRE(dm == nullptr || inv_calibration9 != nullptr, "null argument");
    return sgm_init_depth(ctx, dm, dm_w, dm_h, inv_calibration9, dm_is_z_depth != 0 ? 1 : 0, sigma,
        kernel_size, out);
}

static int
sgm_init_depth(smvs_ctx *ctx, const float *dm, int dm_w, int dm_h, const float *inv_calibration9,
    int dm_is_z_depth, float sigma, int kernel_size, float *out)
{
    SMVS_REQUIRE(ctx != nullptr, "null argument");
    if (dm == nullptr) {   // forget the resident map
        ctx->sgm_resident = false;
        ctx->sgm_slant_ok = false;
        return SMVS_OK;
    }
    SMVS_REQUIRE(dm_w > 0 && dm_h > 0 && kernel_size >= 0 && sigma > 0.f,
        "bad argument");
    if ((ctx->image_ok & 1u) == 0u) {
        set_error("smvs_ctx_sgm_init_depth: no main image (smvs_ctx_upload_image)");
        return SMVS_ERR_STATE;
    }
    if (ctx->images[0].w != ctx->width || ctx->images[0].h != ctx->height) {
        set_error("smvs_ctx_sgm_init_depth: main image size differs from the context");
        return SMVS_ERR_INVALID;
    }
    SMVS_HIP_CHECK(set_device(ctx->device));
    int rc;
    // (the guide image may still be on its way: smvs_ctx_upload_image_async)
    if ((rc = ctx_materialise_images(ctx, 1u)) != SMVS_OK)
        return rc;
    size_t const n = (size_t)ctx->width * ctx->height;
    size_t const n_low = (size_t)dm_w * dm_h;
    if (ctx->sgm_lowres_cap < n_low) {
        if ((rc = device_alloc(&ctx->sgm_lowres, n_low)) != SMVS_OK)
            return rc;
        ctx->sgm_lowres_cap = n_low;
    }
    if (ctx->topo_sgm_cap < n) {
        if ((rc = device_alloc(&ctx->topo_sgm, n)) != SMVS_OK)
            return rc;
        ctx->topo_sgm_cap = n;
    }
    ctx->sgm_resident = false;
    ctx->sgm_slant_ok = false;   // (a new map invalidates the slant plane)
    ctx->sgm_lowres_w = dm_w;
    ctx->sgm_lowres_h = dm_h;
    {
        // The map goes to the device through a kernel that reads page-locked
        // memory over the bus, not as a DMA: at this moment the nine images of the
        // view are on their way (smvs_ctx_upload_image_async) and a tenth transfer
        // queues behind them, with the host waiting for it before it can launch
        // the filter (round 6, profiles/r6_upload_overlap.txt).
        if (ctx->sgm_pin_busy) {
            SMVS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
            ctx->sgm_pin_busy = false;
        }
        if (ctx->sgm_pin_cap < n_low) {
            if (ctx->sgm_pin != nullptr)
                (void)hipHostFree(ctx->sgm_pin);
            ctx->sgm_pin = nullptr;
            ctx->sgm_pin_cap = 0;
            SMVS_HIP_CHECK(hipHostMalloc(reinterpret_cast<void **>(&ctx->sgm_pin),
                sizeof(float) * n_low, hipHostMallocDefault));
            ctx->sgm_pin_cap = n_low;
        }
        std::memcpy(ctx->sgm_pin, dm, sizeof(float) * n_low);
        SgmMapUpload U;
        U.src = ctx->sgm_pin;
        U.dst = ctx->sgm_lowres;
        U.w = dm_w;
        U.h = dm_h;
        U.from_mve = inv_calibration9 != nullptr ? (dm_is_z_depth ? 2 : 1) : 0;
        for (int i = 0; i < 9; ++i)
            U.invproj[i] = inv_calibration9 != nullptr ? inv_calibration9[i] : 0.0f;
        hipLaunchKernelGGL(sgm_map_upload_kernel, dim3((unsigned)((n_low + 255) / 256)),
            dim3(256), 0, ctx->stream, U);
        SMVS_HIP_CHECK(hipGetLastError());
        ctx->sgm_pin_busy = true;
    }
    BilateralArgs A;
    A.dm = ctx->sgm_lowres;
    A.ci = ctx->images[0].data;
    A.out = ctx->topo_sgm;
    A.dm_w = dm_w;
    A.dm_h = dm_h;
    A.w = ctx->width;
    A.h = ctx->height;
    A.channels = ctx->images[0].c;
    A.kernel_size = kernel_size;
    A.sigma = sigma;
    SgmProfile prof;
    const uint32_t *host_table = nullptr;
    if (kernel_size <= BIL_MAX_K && (A.channels == 1 || A.channels == 3))
        host_table = bilateral_colour_table();
    bool const tabled = host_table != nullptr;
    // the triangle of all pairs in LDS (round 6), unless SMVS_BILATERAL=compressed
    const float *host_triangle = nullptr;
    if (tabled && kernel_size == BIL_TRI_K) {
        const char *form = std::getenv("SMVS_BILATERAL");
        if (!(form != nullptr && std::strcmp(form, "compressed") == 0))
            host_triangle = bilateral_colour_triangle();
    }
    BilateralSpatial S = {};
    size_t const n_img = n * (size_t)A.channels;
    if (tabled) {
#pragma clang fp contract(off)
        if (host_triangle != nullptr) {
            if (ctx->bil_tri == nullptr) {
                if ((rc = device_alloc(&ctx->bil_tri, BIL_TRI_FLOATS)) != SMVS_OK
                    || (rc = ctx_upload(ctx, ctx->bil_tri, host_triangle,
                            BIL_TRI_FLOATS * sizeof(float))) != SMVS_OK) {
                    (void)device_alloc(&ctx->bil_tri, 0);
                    return rc;
                }
            }
        } else if (ctx->bil_lut == nullptr) {
            if ((rc = device_alloc(&ctx->bil_lut, BIL_TABLE_WORDS)) != SMVS_OK
                || (rc = ctx_upload(ctx, ctx->bil_lut, host_table,
                        BIL_TABLE_WORDS * sizeof(uint32_t))) != SMVS_OK)
                return rc;
        }
        // (the byte staging buffer of the image uploads is free between them)
        if (ctx->byte_stage_cap < n_img) {
            if ((rc = device_alloc(&ctx->byte_stage, n_img)) != SMVS_OK) {
                ctx->byte_stage_cap = 0;
                return rc;
            }
            ctx->byte_stage_cap = n_img;
        }
        // math::gaussian_2d as bilateral_kernel evaluates it, with the host's expf
        int const kw = 2 * kernel_size + 1;
        for (int ky = -kernel_size; ky <= kernel_size; ++ky)
            for (int kx = -kernel_size; kx <= kernel_size; ++kx)
                S.w[(ky + kernel_size) * kw + (kx + kernel_size)]
                    = expf(-((float)kx * (float)kx / (2.0f * sigma * sigma)
                        + (float)ky * (float)ky / (2.0f * sigma * sigma)));
    }
    {
        SgmKernelTimer timer(&prof, ctx->stream, SMVS_SGM_K_BILATERAL);
        dim3 const grid((ctx->width + 255) / 256, ctx->height);
        if (tabled) {
            hipLaunchKernelGGL(float_to_byte_kernel, dim3((unsigned)((n_img + 255) / 256)),
                dim3(256), 0, ctx->stream, ctx->images[0].data, ctx->byte_stage, n_img);
            const uint32_t *table = reinterpret_cast<const uint32_t *>(ctx->bil_lut);
            if (host_triangle != nullptr) {
                // one workgroup per CU, the table in its LDS for the whole image
                size_t const lds = BIL_TRI_FLOATS * sizeof(float);
                const void *k = A.channels == 3
                    ? reinterpret_cast<const void *>(&bilateral_triangle_kernel<3>)
                    : reinterpret_cast<const void *>(&bilateral_triangle_kernel<1>);
                if ((rc = allow_dynamic_lds(ctx->device, k, lds)) != SMVS_OK)
                    return rc;
                int cus = 0;
                if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount,
                        physical_device(ctx->device)) != hipSuccess || cus <= 0)
                    cus = 256;
                unsigned const blocks = (unsigned)std::min<size_t>((size_t)cus,
                    (n + BIL_TRI_THREADS - 1) / BIL_TRI_THREADS);
                if (A.channels == 3)
                    hipLaunchKernelGGL(bilateral_triangle_kernel<3>, dim3(blocks),
                        dim3(BIL_TRI_THREADS), lds, ctx->stream, A, ctx->byte_stage, ctx->bil_tri, S);
                else
                    hipLaunchKernelGGL(bilateral_triangle_kernel<1>, dim3(blocks),
                        dim3(BIL_TRI_THREADS), lds, ctx->stream, A, ctx->byte_stage, ctx->bil_tri, S);
            } else if (A.channels == 3)
                hipLaunchKernelGGL(bilateral_table_kernel<3>, grid, dim3(256), 0, ctx->stream,
                    A, ctx->byte_stage, table, S);
            else
                hipLaunchKernelGGL(bilateral_table_kernel<1>, grid, dim3(256), 0, ctx->stream,
                    A, ctx->byte_stage, table, S);
        } else {
            hipLaunchKernelGGL(bilateral_kernel, grid, dim3(256), 0, ctx->stream, A);
        }
    }
    SMVS_HIP_CHECK(hipGetLastError());
    // (no wait when the caller does not want the filtered map back: whatever
    // reads it next runs behind the filter on the context's stream)
    if (out != nullptr) {
        if ((rc = ctx_download(ctx, out, ctx->topo_sgm, sizeof(float) * n)) != SMVS_OK)
            return rc;
        ctx->sgm_pin_busy = false;
    }
    ctx->sgm_resident = true;
    return SMVS_OK;
}

