// Undistortion resampling on gfx950 (smvs_undistort_u8, include/smvs_hip.h):
// an interleaved u8 image of a camera with radial / tangential distortion, an
// off-centre principal point or non-square pixels is resampled into the pinhole
// camera the rest of the library works with (centred principal point, square
// pixels: CameraInfo carries only flen).  The per-pixel arithmetic is
// host/undistort_math.h, shared with the host form (host/colmap_io.cc).
#include "sgm_internal.h"

#include <cmath>

#include "host/undistort_math.h"

using namespace smvs_hip;
using namespace smvs_undistort;

// The kernel is a gather: output pixel (x, y) reads the 2 x 2 source pixels
// around its source position, and for the lenses this is meant for the source
// window of an output tile is the tile itself, bent a little.  A workgroup
// makes a tile of UND_TX x UND_TY output pixels, so that the source rows one
// output row reads are read again by the next output row of the same workgroup
// out of the CU's L1 / the L2, not from HBM.
//
// A lane makes one aligned dword of an output row at a time (a run of 4 / C
// pixels) and stores it whole.  An output row starts at any byte (w * 3 with
// odd w), so the first and the last dword of a tile's row segment can be shared
// with the neighbouring tile or the next row: those are stored byte by byte,
// each byte by the tile that owns it.  The position and the taps are formed
// once per pixel, not once per byte.  The taps are byte loads: neighbouring
// lanes read neighbouring source bytes, and a byte is read by four output
// pixels, all from the same or the next tile row.
//
// Blank pixels (outside the source image) are counted where the pixel's first
// byte is made: per lane, summed over the wave, over the workgroup's four waves
// in LDS, one 64-bit integer atomic per workgroup that has any.
constexpr int UND_TX = 64;
constexpr int UND_TY = 16;

template <int C>
__global__ void __launch_bounds__(256)
undistort_u8_kernel(const uint8_t *__restrict__ src, Mapping m, int ow, int oh,
    uint8_t *__restrict__ out, unsigned long long *__restrict__ blank)
{
#pragma clang fp contract(off)
    constexpr int OUT_DW = UND_TX * C / 4 + 1;   // dwords a row segment of the tile can touch
    __shared__ unsigned wave_blank[4];
    int const tid = threadIdx.x;
    int const tx0 = blockIdx.x * UND_TX, ty0 = blockIdx.y * UND_TY;
    int const tx1 = min(tx0 + UND_TX, ow), ty1 = min(ty0 + UND_TY, oh);   // exclusive
    size_t const orow = (size_t)ow * C;
    unsigned nblank = 0;
    for (int idx = tid; idx < (ty1 - ty0) * OUT_DW; idx += 256) {
        int const yy = idx / OUT_DW, q = idx - yy * OUT_DW;
        int const y = ty0 + yy;
        size_t const row0 = (size_t)y * orow;
        size_t const gs = row0 + (size_t)tx0 * C, ge = row0 + (size_t)tx1 * C;
        size_t const g0 = ((gs >> 2) + (size_t)q) << 2;
        if (g0 >= ge)
            continue;
        uint32_t packed = 0;
        bool all = true;
        int cur_x = -1;
        bool inside = false;
        Taps taps = {};
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            size_t const g = g0 + (size_t)b;
            bool const valid = g >= gs && g < ge;
            all = all && valid;
            if (!valid)
                continue;
            int const j = (int)(g - row0);
            int const x = j / C, ch = j - x * C;
            if (x != cur_x) {
                cur_x = x;
                float sx, sy;
                inside = source_position(m, x, y, &sx, &sy);
                if (inside)
                    taps = make_taps(m, C, sx, sy);
                else if (ch == 0)
                    nblank += 1;
            }
            uint32_t const byte = inside ? (uint32_t)sample(src, taps, ch) : 0u;
            packed |= byte << (8 * b);
        }
        if (all) {
            *reinterpret_cast<uint32_t *>(out + g0) = packed;
        } else {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (g0 + (size_t)b >= gs && g0 + (size_t)b < ge)
                    out[g0 + (size_t)b] = (uint8_t)(packed >> (8 * b));
        }
    }
    // (every lane arrives here: the loop leaves by its condition only)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        nblank += __shfl_xor(nblank, off, 64);
    if ((tid & 63) == 0)
        wave_blank[tid >> 6] = nblank;
    __syncthreads();
    if (tid == 0) {
        unsigned const total = wave_blank[0] + wave_blank[1] + wave_blank[2] + wave_blank[3];
        if (total != 0)
            atomicAdd(blank, (unsigned long long)total);
    }
}

template <int C>
static void
launch_undistort(const uint8_t *src, Mapping const &m, int ow, int oh, uint8_t *out,
    unsigned long long *blank, hipStream_t stream)
{
    hipLaunchKernelGGL(undistort_u8_kernel<C>,
        dim3((unsigned)((ow + UND_TX - 1) / UND_TX), (unsigned)((oh + UND_TY - 1) / UND_TY)),
        dim3(256), 0, stream, src, m, ow, oh, out, blank);
}

static bool
undistort_size_ok(int w, int h, int channels)
{
    return w <= (1 << 20) && h <= (1 << 20)
        && (size_t)w * (size_t)h * (size_t)channels <= ((size_t)1 << 31);
}

extern "C" int
smvs_undistort_u8(int device, const uint8_t *pixels, int width, int height, int channels,
    const smvs_lens *lens, float out_focal, int out_width, int out_height, uint8_t *out,
    int64_t *blank_pixels)
{
    SMVS_REQUIRE(pixels && lens && out, "null argument");
    SMVS_REQUIRE(channels >= 1 && channels <= 4, "1 to 4 channels");
    SMVS_REQUIRE(width >= 1 && height >= 1 && out_width >= 1 && out_height >= 1,
        "a size below 1");
    SMVS_REQUIRE(out_focal > 0.0f && std::isfinite(out_focal),
        "out_focal must be positive and finite");
    SMVS_REQUIRE(std::isfinite(lens->fx) && std::isfinite(lens->fy) && std::isfinite(lens->cx)
        && std::isfinite(lens->cy) && std::isfinite(lens->k1) && std::isfinite(lens->k2)
        && std::isfinite(lens->p1) && std::isfinite(lens->p2), "non-finite lens value");
    SMVS_REQUIRE(undistort_size_ok(width, height, channels)
        && undistort_size_ok(out_width, out_height, channels), "image too large");
    Mapping const m = make_mapping(lens->fx, lens->fy, lens->cx, lens->cy, lens->k1, lens->k2,
        lens->p1, lens->p2, width, height, out_focal, out_width, out_height);
    WorkspaceLease lease(device);
    if (lease.w == nullptr)
        return SMVS_ERR_HIP;
    Workspace &ws = *lease.w;
    int rc;
    size_t const in_bytes = (size_t)width * height * channels;
    size_t const out_bytes = (size_t)out_width * out_height * channels;
    // the blank counter sits behind the output, 8-byte aligned
    size_t const counter_at = (out_bytes + 7) & ~(size_t)7;
    uint8_t *d_in = nullptr, *d_out = nullptr;
    if ((rc = ws.ensure(WS_RAW, in_bytes, &d_in))
        || (rc = ws.ensure(WS_RAW0, counter_at + 8, &d_out))
        || (rc = ws.upload(d_in, pixels, in_bytes)))
        return rc;
    unsigned long long *d_blank = reinterpret_cast<unsigned long long *>(d_out + counter_at);
    SMVS_HIP_CHECK(hipMemsetAsync(d_blank, 0, 8, ws.stream));
    switch (channels) {
    case 1: launch_undistort<1>(d_in, m, out_width, out_height, d_out, d_blank, ws.stream); break;
    case 2: launch_undistort<2>(d_in, m, out_width, out_height, d_out, d_blank, ws.stream); break;
    case 3: launch_undistort<3>(d_in, m, out_width, out_height, d_out, d_blank, ws.stream); break;
    default: launch_undistort<4>(d_in, m, out_width, out_height, d_out, d_blank, ws.stream); break;
    }
    SMVS_HIP_CHECK(hipGetLastError());
    if ((rc = ws.download(out, d_out, out_bytes)) != SMVS_OK)
        return rc;
    if (blank_pixels != nullptr) {
        unsigned long long n = 0;
        if ((rc = ws.download(&n, d_blank, 8)) != SMVS_OK)
            return rc;
        *blank_pixels = (int64_t)n;
    }
    return SMVS_OK;
}
