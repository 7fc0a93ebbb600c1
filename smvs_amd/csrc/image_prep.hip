// Image preparation on gfx950: a view's SGM input image (desaturate, half-size
// steps) and the scene's input scaling (chained half-size Gaussian,
// smvs_rescale_half_gaussian).
#include "sgm_internal.h"

#include <cmath>

using namespace smvs_hip;

// StereoView::get_byte_image (desaturate<uint8_t>, stereo_view.cc:86-95
// [MVE-unverified]: 0.21 r + 0.72 g + 0.07 b + 0.5, truncated) on the device
__global__ void __launch_bounds__(256)
sgm_desaturate_kernel(const uint8_t *__restrict__ in, size_t npix, int channels,
    uint8_t *__restrict__ out)
{
#pragma clang fp contract(off)
    size_t const p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix)
        return;
    if (channels < 3) {
        out[p] = in[p * channels];
        return;
    }
    float const v = (float)in[p * channels] * 0.21f + (float)in[p * channels + 1] * 0.72f
        + (float)in[p * channels + 2] * 0.07f + 0.5f;
    out[p] = (uint8_t)v;
}

// mve::image::rescale_half_size<uint8_t> (sgm_stereo.cc:31-39 [MVE-unverified]):
// mean of the 2 x 2 block (odd sizes repeat the last row / column), + 0.5, truncated
__global__ void __launch_bounds__(256)
sgm_half_size_kernel(const uint8_t *__restrict__ in, int w, int h,
    uint8_t *__restrict__ out)
{
#pragma clang fp contract(off)
    int const ow = (w + 1) >> 1, oh = (h + 1) >> 1;
    int const x = blockIdx.x * blockDim.x + threadIdx.x;
    int const y = blockIdx.y;
    if (x >= ow || y >= oh)
        return;
    int const x0 = 2 * x, x1 = min(2 * x + 1, w - 1);
    int const y0 = 2 * y, y1 = min(2 * y + 1, h - 1);
    float const v = (float)in[(size_t)y0 * w + x0] * 0.25f
        + (float)in[(size_t)y0 * w + x1] * 0.25f
        + (float)in[(size_t)y1 * w + x0] * 0.25f
        + (float)in[(size_t)y1 * w + x1] * 0.25f;
    out[(size_t)y * ow + x] = (uint8_t)(v + 0.5f);
}

// mve::image::rescale_half_size_gaussian<uint8_t>(img, sigma2 = 0.75f)
// [MVE-unverified M29], the input scaling of app/smvsrecon.cc:634-647, with the
// bits of the host mirror's loop (host/scene_io.cc, rescale_half_size_gaussian):
// interleaved u8 [h][w][C] -> ((w + 1) / 2, (h + 1) / 2, C); output (x, y) reads
// the rows max(0, 2y - 1), 2y, min(h - 1, 2y + 1), min(h - 1, 2y + 2) and the
// columns by the same rule.
//
// What makes the result the host's, bit for bit:
//   weights       w1, w2, w3 are kernel arguments: the host's std::exp values,
//                 never expf on the device;
//   weight sum    clamping changes which byte a tap reads, not which weight it
//                 adds, so the sum of the sixteen weights is the same at every
//                 position: formed once on the host in the loop's order (wsum);
//   contraction   off: every product is rounded before it is added;
//   order         v = 0, then += (float)byte * weight over the rows and inside
//                 a row over the columns, one chain of sixteen float adds;
//   division      __fdiv_rn: the correctly rounded IEEE quotient (v_div_scale /
//                 v_div_fmas / v_div_fixup), whatever the translation unit's
//                 fast-math or -fhip-fp32-correctly-rounded-divide-sqrt setting;
//   rounding      half away from zero as the host writes it (floor(q + 0.5) for
//                 q > 0, else ceil(q - 0.5)), then the cast to u8.
//
// A workgroup makes an output tile of TX x RHG_TY pixels, TX * C <= 256 bytes
// wide.  Its input -- 2 TX + 2 columns by 2 RHG_TY + 2 rows, the tile times two
// plus the apron of one pixel before and two behind -- is staged in LDS with
// aligned dword loads along the interleaved rows, so that a byte comes from HBM
// once (1 / 64 + 1 / 16 more for the aprons, which the L2 serves).  A row of the
// image starts at any byte, so row r of the tile is stored from the aligned
// dword below its first byte and read back with that row's shift (0..3).  The
// taps are LDS byte reads; neighbouring lanes make neighbouring output dwords,
// 8 input bytes apart: lanes l and l + 16 of a half wave meet on a bank (2-way).
// Each thread makes one aligned dword of an output row and stores it whole; the
// dwords a tile shares with its neighbour or with the next row (the first and
// the last of a row segment) are stored byte by byte.
constexpr int RHG_TY = 16;
constexpr int RHG_PITCH_DW = 132;   // (2 * 64 + 2) * 4 bytes + 3 of shift, in dwords
template <int C> struct RhgTile { static constexpr int TX = C == 1 ? 256 : C == 2 ? 128 : 64; };

struct RhgArgs {
    const uint8_t *in;     // 4-byte aligned, readable up to the dword that holds the last byte
    uint8_t *out;          // 4-byte aligned
    int w, h, ow, oh;
    float w1, w2, w3, wsum;
};

template <int C>
__global__ void __launch_bounds__(256)
rescale_half_gaussian_u8_kernel(RhgArgs A)
{
#pragma clang fp contract(off)
    constexpr int TX = RhgTile<C>::TX;
    constexpr int OUT_DW = TX * C / 4 + 1;   // dwords a row segment of the tile can touch
    __shared__ uint32_t tile[(2 * RHG_TY + 2) * RHG_PITCH_DW];
    int const tid = threadIdx.x;
    int const tx0 = blockIdx.x * TX, ty0 = blockIdx.y * RHG_TY;
    int const tx1 = min(tx0 + TX, A.ow), ty1 = min(ty0 + RHG_TY, A.oh);   // exclusive
    // staged input pixels [xin0, xin1] x [yin0, yin1]
    int const xin0 = max(0, 2 * tx0 - 1), xin1 = min(A.w - 1, 2 * tx1);
    int const yin0 = max(0, 2 * ty0 - 1), yin1 = min(A.h - 1, 2 * ty1);
    int const nrows = yin1 - yin0 + 1;
    int const nbytes = (xin1 - xin0 + 1) * C;          // <= (2 TX + 2) C <= 520
    size_t const rowbytes = (size_t)A.w * C;
    size_t const in_dwords = (rowbytes * (size_t)A.h + 3) >> 2;
    const uint32_t *in32 = reinterpret_cast<const uint32_t *>(A.in);
    for (int idx = tid; idx < nrows * RHG_PITCH_DW; idx += 256) {
        int const r = idx / RHG_PITCH_DW, d = idx - r * RHG_PITCH_DW;
        size_t const first = (size_t)(yin0 + r) * rowbytes + (size_t)xin0 * C;
        size_t const dw = (first >> 2) + (size_t)d;
        // (the dwords that hold bytes of this row of the tile, inside the buffer)
        if (dw <= ((first + (size_t)nbytes - 1) >> 2) && dw < in_dwords)
            tile[idx] = in32[dw];
    }
    __syncthreads();
    const uint8_t *tb = reinterpret_cast<const uint8_t *>(tile);
    int const shift_mul = (int)(rowbytes & 3), shift_add = (xin0 * C) & 3;
    size_t const orow = (size_t)A.ow * C;
    float const wk[4] = { A.w2, A.w1, A.w1, A.w2 };   // rows 1, 2; rows 0, 3 below
    float const we[4] = { A.w3, A.w2, A.w2, A.w3 };
    for (int idx = tid; idx < (ty1 - ty0) * OUT_DW; idx += 256) {
        int const yy = idx / OUT_DW, q = idx - yy * OUT_DW;
        int const y = ty0 + yy;
        size_t const row0 = (size_t)y * orow;
        size_t const gs = row0 + (size_t)tx0 * C, ge = row0 + (size_t)tx1 * C;
        size_t const g0 = ((gs >> 2) + (size_t)q) << 2;
        if (g0 >= ge)
            continue;
        // LDS byte offsets of the four input rows
        int rowoff[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            int const yi = min(A.h - 1, max(0, 2 * y - 1 + r));
            rowoff[r] = (yi - yin0) * (RHG_PITCH_DW * 4)
                + ((((yi & 3) * shift_mul) + shift_add) & 3);
        }
        uint32_t packed = 0;
        bool all = true;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            size_t const g = g0 + (size_t)b;
            bool const valid = g >= gs && g < ge;
            all = all && valid;
            if (!valid)
                continue;
            int const j = (int)(g - row0);
            int const x = j / C, ch = j - x * C;
            int coloff[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                coloff[k] = (min(A.w - 1, max(0, 2 * x - 1 + k)) - xin0) * C + ch;
            float v = 0.0f;
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    v += (float)tb[rowoff[r] + coloff[k]]
                        * ((r == 0 || r == 3) ? we[k] : wk[k]);
            float const quot = __fdiv_rn(v, A.wsum);
            uint8_t const byte = (uint8_t)(quot > 0.0f ? floorf(quot + 0.5f)
                                                       : ceilf(quot - 0.5f));
            packed |= (uint32_t)byte << (8 * b);
        }
        if (all) {
            *reinterpret_cast<uint32_t *>(A.out + g0) = packed;
        } else {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (g0 + (size_t)b >= gs && g0 + (size_t)b < ge)
                    A.out[g0 + (size_t)b] = (uint8_t)(packed >> (8 * b));
        }
    }
}

// one level: a workgroup per tile of RhgTile<C>::TX x RHG_TY output pixels
template <int C>
static void
launch_rescale_half_gaussian(RhgArgs const &A, hipStream_t stream)
{
    constexpr int TX = RhgTile<C>::TX;
    hipLaunchKernelGGL(rescale_half_gaussian_u8_kernel<C>,
        dim3((unsigned)((A.ow + TX - 1) / TX), (unsigned)((A.oh + RHG_TY - 1) / RHG_TY)),
        dim3(256), 0, stream, A);
}

// The levels an image of w x h goes through in `halvings` steps; false when a
// level's input is narrower or lower than 2 (the host function's "image too
// small").  *ow / *oh: the last level's size.
static bool
rescale_half_gaussian_sizes(int w, int h, int halvings, int *ow, int *oh)
{
    for (int i = 0; i < halvings; ++i) {
        if (w < 2 || h < 2)
            return false;
        w = (w + 1) >> 1;
        h = (h + 1) >> 1;
    }
    *ow = w;
    *oh = h;
    return true;
}

// app/smvsrecon.cc:634-647: `halvings` chained rescale_half_size_gaussian of one
// image; the levels ping-pong between two slots of the workspace
extern "C" int
smvs_rescale_half_gaussian(int device, const uint8_t *pixels, int width, int height,
    int channels, int halvings, uint8_t *out, size_t out_capacity, int *out_width,
    int *out_height)
{
    SMVS_REQUIRE(pixels && out && out_width && out_height, "null argument");
    SMVS_REQUIRE(halvings >= 1 && halvings <= 30, "halvings must be in [1, 30]");
    SMVS_REQUIRE(channels >= 1 && channels <= 4, "1 to 4 channels");
    SMVS_REQUIRE(width <= (1 << 20) && height <= (1 << 20)
        && (width < 1 || height < 1
            || (size_t)width * (size_t)height * (size_t)channels <= ((size_t)1 << 31)),
        "image too large");
    int fw = 0, fh = 0;
    SMVS_REQUIRE(rescale_half_gaussian_sizes(width, height, halvings, &fw, &fh),
        "image too small");
    size_t const out_bytes = (size_t)fw * fh * channels;
    SMVS_REQUIRE(out_capacity >= out_bytes, "output buffer too small");
    // the host's weights and their sum in the host loop's order (scene_io.cc)
    float const sigma2 = 0.75f;
    float const w1 = std::exp(-0.5f / (2.0f * sigma2));
    float const w2 = std::exp(-2.5f / (2.0f * sigma2));
    float const w3 = std::exp(-4.5f / (2.0f * sigma2));
    float const wrow[4][4] = { { w3, w2, w2, w3 }, { w2, w1, w1, w2 },
        { w2, w1, w1, w2 }, { w3, w2, w2, w3 } };
    float wsum = 0.0f;
    {
#pragma clang fp contract(off)
        for (int r = 0; r < 4; ++r)
            for (int k = 0; k < 4; ++k)
                wsum += wrow[r][k];
    }
    WorkspaceLease lease(device);
    if (lease.w == nullptr)
        return SMVS_ERR_HIP;
    Workspace &ws = *lease.w;
    int rc;
    size_t const in_bytes = (size_t)width * height * channels;
    size_t const half_bytes = (size_t)((width + 1) >> 1) * ((height + 1) >> 1) * channels;
    uint8_t *cur = nullptr, *other = nullptr;
    // (whole dwords: the kernel loads the dword that holds a level's last byte)
    if ((rc = ws.ensure(WS_RAW, (in_bytes + 3) & ~(size_t)3, &cur))
        || (rc = ws.ensure(WS_RAW0, (half_bytes + 3) & ~(size_t)3, &other))
        || (rc = ws.upload(cur, pixels, in_bytes)))
        return rc;
    int cw = width, ch = height;
    for (int i = 0; i < halvings; ++i) {
        RhgArgs A;
        A.in = cur;
        A.out = other;
        A.w = cw;
        A.h = ch;
        A.ow = (cw + 1) >> 1;
        A.oh = (ch + 1) >> 1;
        A.w1 = w1;
        A.w2 = w2;
        A.w3 = w3;
        A.wsum = wsum;
        switch (channels) {
        case 1: launch_rescale_half_gaussian<1>(A, ws.stream); break;
        case 2: launch_rescale_half_gaussian<2>(A, ws.stream); break;
        case 3: launch_rescale_half_gaussian<3>(A, ws.stream); break;
        default: launch_rescale_half_gaussian<4>(A, ws.stream); break;
        }
        SMVS_HIP_CHECK(hipGetLastError());
        uint8_t *t = cur; cur = other; other = t;
        cw = A.ow;
        ch = A.oh;
    }
    if ((rc = ws.download(out, cur, out_bytes)) != SMVS_OK)
        return rc;
    *out_width = cw;
    *out_height = ch;
    return SMVS_OK;
}

// (declared in sgm_internal.h)
smvs_hip::SgmPreparedSize
smvs_hip::sgm_prepared_size(int w, int h, int channels, int halvings)
{
    size_t const npix = (size_t)w * h;
    // raw bytes and the grey image behind them; neither for an image that is
    // one channel at SGM scale already
    SgmPreparedSize Z = { w, h, npix,
        channels == 1 && halvings == 0 ? 0 : npix * (size_t)channels + npix };
    for (int i = 0; i < halvings; ++i) {
        Z.w = (Z.w + 1) >> 1;
        Z.h = (Z.h + 1) >> 1;
    }
    return Z;
}

// (declared in sgm_internal.h)
int
smvs_hip::sgm_prepare_image(Workspace &ws, const uint8_t *host, int w, int h, int channels,
    int halvings, int slot_out, int slot_tmp, uint8_t **out, int *ow, int *oh)
{
    int rc;
    SgmPreparedSize const Z = sgm_prepared_size(w, h, channels, halvings);
    size_t const npix = (size_t)w * h;
    uint8_t *a = nullptr, *b = nullptr;
    *ow = Z.w;
    *oh = Z.h;
    if (Z.tmp == 0) {
        if ((rc = ws.ensure(slot_out, Z.out, &a)) || (rc = ws.upload(a, host, npix)))
            return rc;
        *out = a;
        return SMVS_OK;
    }
    // raw bytes into the scratch slot, results ping-pong between the two
    if ((rc = ws.ensure(slot_tmp, Z.tmp, &b))
        || (rc = ws.ensure(slot_out, Z.out, &a))
        || (rc = ws.upload(b, host, npix * (size_t)channels)))
        return rc;
    uint8_t *grey = b + npix * (size_t)channels;   // behind the raw bytes
    hipLaunchKernelGGL(sgm_desaturate_kernel, dim3((unsigned)((npix + 255) / 256)),
        dim3(256), 0, ws.stream, b, npix, channels, halvings % 2 == 0 ? a : grey);
    uint8_t *cur = halvings % 2 == 0 ? a : grey;
    uint8_t *other = halvings % 2 == 0 ? grey : a;
    int cw = w, ch = h;
    for (int i = 0; i < halvings; ++i) {
        int const nw = (cw + 1) >> 1, nh = (ch + 1) >> 1;
        hipLaunchKernelGGL(sgm_half_size_kernel, dim3((nw + 255) / 256, nh), dim3(256), 0,
            ws.stream, cur, cw, ch, other);
        uint8_t *t = cur; cur = other; other = t;
        cw = nw;
        ch = nh;
    }
    SMVS_HIP_CHECK(hipGetLastError());
    // (an even number of swaps ends in `a` when it started there, an odd one
    // when it started in `grey`: cur == a by construction)
    *out = cur;
    return SMVS_OK;
}
