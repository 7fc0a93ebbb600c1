// Census / plane-sweep cost volume, 8-path SGM aggregation and WTA on gfx950:
// one run_sgm, as smvs_sgm_run[_mode] and as sgm_run_device for a view's front
// end (sgm_view.hip); and the counters of the front end's kernel timer.
//
// Replaces SGMStereo::run_sgm (reference: lib/sgm_stereo.cc:98-124):
// census_filter (:126-148), warped_neighbors_for_depth (:150-190),
// create_cost_volume (:192-244), aggregate_sgm_costs (:429-667, the SSE
// branch with constant penalty2, :361-406; on request the branch without SSE,
// fill_path_cost :310-346 with its seeds :626-654 -- SMVS_SGM_P2_ADAPTIVE, the
// ADAPT kernels below), depth_from_sgm_volume (:274-306).
//
// Integer path: results are bit-exact with the reference semantics.  The
// float warp is evaluated in the reference's operation order with FMA
// contraction off.  Volumes are [y][x][d], d fastest (sgm_stereo.cc:436-437);
// the cost volume is kept as u8 (values <= 255), S as u16.
//
// Aggregation: every path direction is an independent 1-D recurrence along a
// row, a column or a diagonal line of the image, so one wavefront walks one
// line (lane l owns planes 2l, 2l+1; neighbours and the minimum by DPP), with
// the loads of the next pixels issued ahead of the dependent chain.  With an
// even plane count all eight directions run in ONE launch and add into S with
// atomics on packed u16 pairs (integer adds commute: bit-exact); odd plane
// counts take one launch per direction.  Each path reads C once and
// read-modify-writes S once.  Plane counts above 128 (multiples of 8 up to
// SGM_MAX_PLANES): sgm_paths_wide_kernel, four planes per lane.
#include "dpp.h"
#include "sgm_internal.h"

#include <cstdlib>
#include <mutex>
#include <type_traits>
#include <utility>

namespace smvs_hip {

// ------------------------------------------------------------------ census
// sgm_stereo.cc:126-148: 9x7 window, x in [4, w-5), y in [3, h-4); bit = centre
// < neighbour, MSB first in (i outer, j inner) order; centre 0 -> census 0.
__global__ void __launch_bounds__(256)
census_main_kernel(const uint8_t *__restrict__ img, int w, int h,
    unsigned long long *__restrict__ out)
{
    int const x = blockIdx.x * blockDim.x + threadIdx.x;
    int const y = blockIdx.y;
    if (x >= w)
        return;
    unsigned long long census = 0;
    if (x >= 4 && x < w - 5 && y >= 3 && y < h - 4) {
        uint8_t const thr = img[(size_t)y * w + x];
        if (thr != 0) {
            for (int i = x - 4; i < x + 5; ++i)
                for (int j = y - 3; j < y + 4; ++j) {
                    census <<= 1;
                    if (thr < img[(size_t)j * w + i])
                        census |= 1ull;
                }
        }
    }
    out[(size_t)y * w + x] = census;
}

struct WarpArgs {
    const uint8_t *neighbor;
    int nw, nh;
    float M[9], t[3];
    const float *depths;
    int D, w, h;
    uint8_t *warped;   // [h][w][D]
};

// sgm_stereo.cc:150-190.  One wavefront = 64 pixels of a row x 64 planes: a
// lane keeps its pixel's M p (plane independent) and walks the planes, so the
// 64 samples of an instruction are neighbours in the neighbour image; the
// bytes go through an LDS tile [pixel][plane] and leave as 64 contiguous
// bytes per pixel.  (One thread per (pixel, plane) spent twice the
// instructions: M p, the plane's depth and the address arithmetic per sample.)
constexpr int WARP_TILE = 64;            // pixels and planes per wave
constexpr int WARP_PITCH = WARP_TILE + 4;   // bytes per pixel row of the tile (17 dwords: no bank conflicts)

__global__ void __launch_bounds__(WARP_TILE)
warp_kernel(WarpArgs A)
{
#pragma clang fp contract(off)
    __shared__ uint8_t tile[WARP_TILE * WARP_PITCH];
    int const lane = (int)threadIdx.x;
    int const x0 = (int)blockIdx.x * WARP_TILE;
    int const x = x0 + lane;
    int const y = (int)blockIdx.y;
    int const dbase = (int)blockIdx.z * WARP_TILE;
    int const nd = min(WARP_TILE, A.D - dbase);
    if (x < A.w) {
        float const px = 0.5f + (float)x, py = 0.5f + (float)y;
        float tp[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            float s = 0.0f;
            s += A.M[3 * r + 0] * px;
            s += A.M[3 * r + 1] * py;
            s += A.M[3 * r + 2] * 1.f;
            tp[r] = s;
        }
        float const xmax = (float)(A.nw - 1), ymax = (float)(A.nh - 1);
#pragma unroll 4
        for (int dd = 0; dd < nd; ++dd) {
            float const depth = A.depths[dbase + dd];
            float p0 = tp[0] * depth + A.t[0];
            float p1 = tp[1] * depth + A.t[1];
            float const p2 = tp[2] * depth + A.t[2];
            uint8_t out = 0;
            if (!(p2 < 0)) {
                p0 /= p2;
                p1 /= p2;
                p0 -= 0.5f;
                p1 -= 0.5f;
                if (!(p0 < 0 || p1 < 0 || p0 > xmax || p1 > ymax)) {
                    // mve::Image<uint8_t>::linear_at [MVE-unverified]
                    float const fx = fmaxf(0.0f, fminf(xmax, p0));
                    float const fy = fmaxf(0.0f, fminf(ymax, p1));
                    int const ix = (int)fx, iy = (int)fy;
                    int const ix1 = min(ix + 1, A.nw - 1), iy1 = min(iy + 1, A.nh - 1);
                    float const w1 = fx - (float)ix, w0 = 1.0f - w1;
                    float const w3 = fy - (float)iy, w2 = 1.0f - w3;
                    const uint8_t *r0 = A.neighbor + (size_t)iy * A.nw;
                    const uint8_t *r1 = A.neighbor + (size_t)iy1 * A.nw;
                    float const v1 = (float)r0[ix];
                    float const v2 = (float)r0[ix1];
                    float const v3 = (float)r1[ix];
                    float const v4 = (float)r1[ix1];
                    out = (uint8_t)(v1 * (w0 * w2) + v2 * (w1 * w2) + v3 * (w0 * w3)
                        + v4 * (w1 * w3) + 0.5f);
                }
            }
            tile[lane * WARP_PITCH + dd] = out;
        }
    }
    __syncthreads();
    // 16 lanes x 4 bytes per pixel, 4 pixels per sweep
    bool const quads = (A.D & 3) == 0;
    for (int idx = lane; idx < WARP_TILE * (WARP_TILE / 4); idx += WARP_TILE) {
        int const pix = idx >> 4, q = idx & 15;
        int const gx = x0 + pix, dd = 4 * q;
        if (gx >= A.w || dd >= nd)
            continue;
        size_t const o = ((size_t)y * A.w + gx) * A.D + dbase + dd;
        const uint8_t *src = tile + pix * WARP_PITCH + dd;
        if (quads) {
            *reinterpret_cast<uint32_t *>(A.warped + o) = *reinterpret_cast<const uint32_t *>(src);
        } else {
            for (int k = 0; k < 4 && dd + k < nd; ++k)
                A.warped[o + k] = src[k];
        }
    }
}

// ---------------------------------------------------------------------------
// The same cost volume with TWO planes per lane in the two 16-bit halves of a
// register and the census window kept in registers (round 5).
//
// cost_tiled_kernel below spends 3 vector instructions and one LDS byte read
// per census bit and plane (63 x 3 x 66 M: the ~410 us it takes).  Two
// observations:
//   * the Hamming distance needs no census word: with the main view's bit m_k
//     (the same for every plane of a pixel, so it lives in scalar registers)
//         popcount(census_warped ^ census_main) = sum_k [thr < v_k] ^ m_k
//                                               = popcount(m) + sum_k s_k [thr < v_k],
//     s_k = +1 where m_k = 0 and -1 where m_k = 1.  Per bit and PAIR of planes:
//     a saturating packed subtraction (v_k - thr, zero unless thr < v_k), a
//     packed minimum with 1, a packed multiply-add with the scalar s_k --
//     three instructions for two planes instead of three for one;
//   * the 9 x 7 windows of neighbouring pixels share eight of their nine
//     columns: a wave that walks a row keeps the window in 63 registers and
//     reads the ONE new column per pixel, 7 LDS reads instead of 63.
// Same tile, same bits (tests/test_gpu_parity.py, test_sgm_bit_exact: cost
// volume array_equal with the oracle); plane counts that are not a multiple
// of four keep the kernel below.
constexpr int CP_W = 16, CP_H = 8, CP_D = 128;

// (written as instructions: from `min(sub_sat(v, thr), 1)` on a 2 x u16 vector
// type the compiler builds compares and selects per half, five instructions
// where these are two)
__device__ __forceinline__ uint32_t
pk_sub_sat_u16(uint32_t a, uint32_t b)
{
    uint32_t r;
    asm("v_pk_sub_u16 %0, %1, %2 clamp" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ uint32_t
pk_min_u16(uint32_t a, uint32_t b)
{
    uint32_t r;
    asm("v_pk_min_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// a * s + c per half, s in a scalar register
__device__ __forceinline__ uint32_t
pk_mad_u16(uint32_t a, uint32_t s, uint32_t c)
{
    uint32_t r;
    asm("v_pk_mad_u16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(s), "v"(c));
    return r;
}
__device__ __forceinline__ uint32_t
pk_mad_u16_vvv(uint32_t a, uint32_t b, uint32_t c)
{
    uint32_t r;
    asm("v_pk_mad_u16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// f(integral_constant<0>), f(integral_constant<1>), ... in order
template <typename F, int... I>
__device__ __forceinline__ void
for_each_index(F &f, std::integer_sequence<int, I...>)
{
    (f(std::integral_constant<int, I>()), ...);
}

__global__ void __launch_bounds__(256)
cost_packed_kernel(const uint8_t *__restrict__ warped,
    const unsigned long long *__restrict__ main_census, int w, int h, int D,
    uint8_t *__restrict__ cost)
{
    constexpr int TW = CP_W + 8;
    __shared__ uint8_t tile[(CP_H + 6) * TW * CP_D];
    int const tiles_x = (w + CP_W - 1) / CP_W;
    // Tiles are dealt to the XCDs in contiguous bands (round 6): a tile stages a
    // (16 + 8) x (8 + 6) window, 2.6 x its own pixels, and with neighbouring tiles
    // on different XCDs (workgroups go round robin) that halo came from HBM every
    // time: 178 MB read per launch for a 66 MB volume (profiles/r6_sgm_counters.txt).
    // The launch is padded to eight bands of equal length.
    unsigned const band = gridDim.x >> 3;
    unsigned const tile_id = (blockIdx.x & 7u) * band + (blockIdx.x >> 3);
    if (tile_id >= (unsigned)(tiles_x * ((h + CP_H - 1) / CP_H)))
        return;
    int const x0 = (int)(tile_id % (unsigned)tiles_x) * CP_W;
    int const y0 = (int)(tile_id / (unsigned)tiles_x) * CP_H;
    int const dbase = blockIdx.y * CP_D;
    int const tid = threadIdx.x;

    // stage: 4 planes (one u32) per thread and position (D is a multiple of 4)
    for (int idx = tid; idx < (CP_H + 6) * TW * (CP_D / 4); idx += 256) {
        int const pos = idx / (CP_D / 4), q = idx - pos * (CP_D / 4);
        int const ty = pos / TW, tx = pos - ty * TW;
        int const gx = x0 - 4 + tx, gy = y0 - 3 + ty;
        int const d4 = dbase + 4 * q;
        uint32_t v = 0;
        if (gx >= 0 && gx < w && gy >= 0 && gy < h && d4 < D)
            v = *reinterpret_cast<const uint32_t *>(warped + ((size_t)gy * w + gx) * D + d4);
        *reinterpret_cast<uint32_t *>(tile + (size_t)pos * CP_D + 4 * q) = v;
    }
    __syncthreads();

    int const lane = tid & 63, wave = tid >> 6;
    int const d0 = dbase + 2 * lane;            // this lane's planes: d0, d0 + 1
    uint32_t const one = 0x00010001u, c255 = 0x00FF00FFu;
    for (int py = wave; py < CP_H; py += 4) {
        int const y = y0 + py;
        if (y >= h)
            break;
        // column c of the tile, rows py .. py + 6: this lane's two planes, one
        // per 16-bit half
        auto load_column = [&](int c, uint32_t (&col)[7]) {
#pragma unroll
            for (int j = 0; j < 7; ++j) {
                uint32_t const raw = *reinterpret_cast<const uint16_t *>(
                    tile + ((py + j) * TW + c) * CP_D + 2 * lane);
                col[j] = (raw & 0xFFu) | ((raw & 0xFF00u) << 8);
            }
        };
        uint32_t win[9][7];
#pragma unroll
        for (int i = 0; i < 9; ++i)
            load_column(i, win[i]);
        // one pixel of the row; PX is a template argument so that every index
        // into the window is a constant and the window stays in registers (a
        // `#pragma unroll` of a loop this long is only partly honoured, and the
        // window then lives in scratch)
        auto pixel = [&](auto px_tag) {
            constexpr int px = decltype(px_tag)::value;
            int const x = x0 + px;
            if (x < w) {
                uint32_t const thr = win[(px + 4) % 9][3];
                unsigned long long const mc = main_census[(size_t)y * w + x];
                // the address is wave-uniform: the bits go to scalar registers
                uint32_t const mhi = __builtin_amdgcn_readfirstlane((uint32_t)(mc >> 32));
                uint32_t const mlo = __builtin_amdgcn_readfirstlane((uint32_t)mc);
                uint32_t const pc = (uint32_t)(__popc(mhi) + __popc(mlo));
                uint32_t c = pc | (pc << 16);
                if (x >= 4 && x < w - 5 && y >= 3 && y < h - 4) {
                    uint32_t cnt = 0u;
                    // sgm_stereo.cc:139-145: i outer, j inner, MSB first: bit k
                    // of the census is bit 62 - k of the 64-bit word
#pragma unroll
                    for (int k = 0; k < 63; ++k) {
                        int const i = k / 7, j = k - 7 * i;
                        if (i == 4 && j == 3)
                            continue;   // the centre: thr < thr never holds
                        uint32_t const v = win[(px + i) % 9][j];
                        uint32_t const lt = pk_min_u16(pk_sub_sat_u16(v, thr), one);
                        int const bit = 62 - k;
                        bool const m = ((bit >= 32 ? mhi >> (bit - 32) : mlo >> bit) & 1u) != 0u;
                        cnt = pk_mad_u16(lt, m ? 0xFFFFFFFFu : 0x00010001u, cnt);
                    }
                    // (mod 2^16 per half; the true value is 0 .. 63)
                    c = pk_mad_u16_vvv(cnt, one, c);
                }
                // a plane that was not warped here (thr = 0) costs 255:
                // c = (c - 255) * [thr > 0] + 255 per half
                uint32_t const warped_here = pk_min_u16(thr, one);
                uint32_t const cm = pk_mad_u16_vvv(c255, 0xFFFFFFFFu, c);     // c - 255
                c = pk_mad_u16_vvv(cm, warped_here, c255);
                if (d0 < D)
                    *reinterpret_cast<uint16_t *>(cost + ((size_t)y * w + x) * D + d0)
                        = (uint16_t)((c & 0xFFu) | ((c >> 8) & 0xFF00u));
            }
            // the column that leaves makes room for the one that enters
            if constexpr (px + 1 < CP_W)
                load_column(px + 9, win[px % 9]);
        };
        for_each_index(pixel, std::make_integer_sequence<int, CP_W>());
    }
}

// Cost volume (sgm_stereo.cc:192-244): census of the warped planes + Hamming
// distance to the main census.  A block stages a (16+8) x (8+6) pixel window of
// 64 planes in LDS (each warped byte is needed by 63 census windows), one
// wavefront walks pixels with its lanes along the plane axis, so LDS reads,
// global loads and the u8 cost stores are all 64 contiguous bytes.
constexpr int CT_W = 16, CT_H = 8, CT_D = 64;

__global__ void __launch_bounds__(256)
cost_tiled_kernel(const uint8_t *__restrict__ warped,
    const unsigned long long *__restrict__ main_census, int w, int h, int D,
    uint8_t *__restrict__ cost)
{
    __shared__ uint8_t tile[(CT_H + 6) * (CT_W + 8) * CT_D];
    int const tiles_x = (w + CT_W - 1) / CT_W;
    int const x0 = (blockIdx.x % tiles_x) * CT_W;
    int const y0 = (blockIdx.x / tiles_x) * CT_H;
    int const dbase = blockIdx.y * CT_D;
    int const tid = threadIdx.x;

    // stage: 4 planes (one u32) per thread and position
    bool const aligned = (D & 3) == 0;
    for (int idx = tid; idx < (CT_H + 6) * (CT_W + 8) * (CT_D / 4); idx += 256) {
        int const pos = idx / (CT_D / 4), q = idx - pos * (CT_D / 4);
        int const ty = pos / (CT_W + 8), tx = pos - ty * (CT_W + 8);
        int const gx = x0 - 4 + tx, gy = y0 - 3 + ty;
        int const d4 = dbase + 4 * q;
        uint32_t v = 0;
        if (gx >= 0 && gx < w && gy >= 0 && gy < h && d4 < D) {
            size_t const o = ((size_t)gy * w + gx) * D + d4;
            if (aligned)
                v = *reinterpret_cast<const uint32_t *>(warped + o);
            else
                for (int k = 0; k < 4 && d4 + k < D; ++k)
                    v |= (uint32_t)warped[o + k] << (8 * k);
        }
        *reinterpret_cast<uint32_t *>(tile + (size_t)pos * CT_D + 4 * q) = v;
    }
    __syncthreads();

    int const lane = tid & 63, wave = tid >> 6;
    int const d = dbase + lane;
    for (int py = wave; py < CT_H; py += 4) {
        int const y = y0 + py;
        if (y >= h)
            break;
        for (int px = 0; px < CT_W; ++px) {
            int const x = x0 + px;
            if (x >= w)
                break;
            const uint8_t *centre = tile + ((py + 3) * (CT_W + 8) + px + 4) * CT_D + lane;
            uint32_t const thr = *centre;
            uint32_t c = 255;
            if (thr != 0) {
                uint32_t hi = 0, lo = 0;
                if (x >= 4 && x < w - 5 && y >= 3 && y < h - 4) {
                    // sgm_stereo.cc:139-145: i outer, j inner, MSB first
#pragma unroll
                    for (int k = 0; k < 63; ++k) {
                        int const i = k / 7, j = k - 7 * i;
                        uint32_t const v = tile[((py + j) * (CT_W + 8) + px + i) * CT_D + lane];
                        uint32_t const lt = thr < v ? 1u : 0u;
                        if (k < 31)
                            hi = (hi << 1) | lt;
                        else
                            lo = (lo << 1) | lt;
                    }
                }
                unsigned long long const mc = main_census[(size_t)y * w + x];
                c = __popc(hi ^ (uint32_t)(mc >> 32)) + __popc(lo ^ (uint32_t)mc);
            }
            if (d < D)
                cost[((size_t)y * w + x) * D + d] = (uint8_t)c;
        }
    }
}

// ------------------------------------------------------------- aggregation
struct PathArgs {
    const uint8_t *cost;
    uint16_t *sgm;
    int w, h, D;
    int dx, dy;        // direction of travel
    uint32_t p1, p2;
    int first;         // 1: S is written, not accumulated
    int last;          // 1: last path, fuse the winner-takes-all
    uint8_t *delta;    // all-paths kernel, DELTA form: eight [h][w][D] u8 volumes
    size_t vol;        // bytes of one of them
    const uint8_t *img; // ADAPT kernels: the main image at SGM scale, [h][w]
};

// The reference's build without SSE (sgm_stereo.cc:310-346) adapts penalty2 to
// the intensity step between a pixel and its predecessor on the path:
// max(P1 * 3 / 2, P2 / (|I - I'| + 1)) in int.  It is the same for every plane
// of the pixel, i.e. uniform over the lanes that hold a line.
__device__ __forceinline__ uint32_t
adapted_penalty2(uint32_t p1, uint32_t p2, uint32_t i_here, uint32_t i_before)
{
    uint32_t const diff = (i_here > i_before ? i_here - i_before : i_before - i_here) + 1u;
    return max(p1 * 3u / 2u, p2 / diff);
}


// One wavefront per line.  Lines: for a horizontal path the rows, for a
// vertical path the columns, for a diagonal path all diagonals that start on
// the entry row or the entry column.
//
// Seeding follows the reference exactly (sgm_stereo.cc:457-464, 511-534,
// 589-612): the first pixel of a line copies C and adds it to S; for a
// diagonal path the corner pixel that lies on both the entry row and the
// entry column is added twice.
//
// ADAPT (the build without SSE): penalty2 per step from the image
// (adapted_penalty2, an exact integer division: this kernel serves the odd
// plane counts and is bound by its scalar accesses), and the corner of an
// UPWARD diagonal sweep starts its line with 2 C, not C (:626-654 seed the path
// volumes with `+=`, row loop and column loop both).  No sum wraps inside
// check_sgm_options' range, so the masks below change nothing there.
template <bool ADAPT>
__global__ void __launch_bounds__(64)
sgm_path_kernel(PathArgs A)
{
    int const lane = threadIdx.x;
    int const line = blockIdx.x;
    int const w = A.w, h = A.h, D = A.D;
    int x, y, len;
    int extra_seed = 0;
    if (A.dy == 0) {            // horizontal: one line per row
        if (line >= h)
            return;
        y = line;
        x = A.dx > 0 ? 0 : w - 1;
        len = w;
    } else if (A.dx == 0) {     // vertical: one line per column
        if (line >= w)
            return;
        x = line;
        y = A.dy > 0 ? 0 : h - 1;
        len = h;
    } else {                    // diagonal
        if (line >= w + h - 1)
            return;
        int const y_entry = A.dy > 0 ? 0 : h - 1;
        int const x_entry = A.dx > 0 ? 0 : w - 1;
        if (line < w) {         // starts on the entry row
            x = line;
            y = y_entry;
            if (x == x_entry)
                extra_seed = 1; // corner: row seed + column seed
        } else {                // starts on the entry column, off the corner
            int const k = line - w + 1;
            x = x_entry;
            y = A.dy > 0 ? k : h - 1 - k;
        }
        int const nx = A.dx > 0 ? w - x : x + 1;
        int const ny = A.dy > 0 ? h - y : y + 1;
        len = min(nx, ny);
    }

    int const d0 = 2 * lane, d1 = 2 * lane + 1;
    bool const ok0 = d0 < D, ok1 = d1 < D;
    uint32_t const BIG = 0xFFFFu;
    uint32_t prev0 = BIG, prev1 = BIG;
    uint32_t i_before = 0;

    for (int s = 0; s < len; ++s, x += A.dx, y += A.dy) {
        size_t const base = ((size_t)y * w + x) * D;
        uint32_t c0 = ok0 ? A.cost[base + d0] : 0u;
        uint32_t c1 = ok1 ? A.cost[base + d1] : 0u;
        uint32_t l0, l1;
        uint32_t p2 = A.p2;
        if (ADAPT) {
            uint32_t const i_here = A.img[(size_t)y * w + x];
            p2 = adapted_penalty2(A.p1, A.p2, i_here, i_before);
            i_before = i_here;
        }
        if (s == 0) {
            l0 = c0;
            l1 = c1;
        } else {
            uint32_t const mn = wave_min_u32(min(prev0, prev1));
            uint32_t const left = (uint32_t)__shfl_up((int)prev1, 1);
            uint32_t const right = (uint32_t)__shfl_down((int)prev0, 1);
            bool const has_left = lane > 0;
            bool const has_right = lane < 63 && d1 + 1 < D;
            uint32_t const far = (mn + p2) & 0xFFFFu;
            // u16 wrapping arithmetic of the SSE code (_mm_add_epi16)
            uint32_t u0 = prev0;
            u0 = min(u0, has_left ? ((left + A.p1) & 0xFFFFu) : BIG);
            u0 = min(u0, ok1 ? ((prev1 + A.p1) & 0xFFFFu) : BIG);
            u0 = min(u0, far);
            uint32_t u1 = prev1;
            u1 = min(u1, (prev0 + A.p1) & 0xFFFFu);
            u1 = min(u1, has_right ? ((right + A.p1) & 0xFFFFu) : BIG);
            u1 = min(u1, far);
            l0 = (c0 + u0 - mn) & 0xFFFFu;
            l1 = (c1 + u1 - mn) & 0xFFFFu;
        }
        uint32_t add0 = l0, add1 = l1;
        if (s == 0 && extra_seed) {
            add0 = (2 * c0) & 0xFFFFu;
            add1 = (2 * c1) & 0xFFFFu;
            if (ADAPT && A.dy < 0) {
                l0 = add0;
                l1 = add1;
            }
        }
        if (ok0) {
            uint32_t const old = A.first ? 0u : A.sgm[base + d0];
            A.sgm[base + d0] = (uint16_t)(old + add0);
        }
        if (ok1) {
            uint32_t const old = A.first ? 0u : A.sgm[base + d1];
            A.sgm[base + d1] = (uint16_t)(old + add1);
        }
        prev0 = ok0 ? l0 : BIG;
        prev1 = ok1 ? l1 : BIG;
    }
}

// Line geometry shared by both path kernels.  Seeding follows the reference
// exactly (sgm_stereo.cc:457-464, 511-534, 589-612): the first pixel of a
// line copies C and adds it to S; for a diagonal path the corner pixel that
// lies on both the entry row and the entry column is added twice (every
// entry-column pixel is the start of its own diagonal, so the reference's
// column seeding needs nothing else).
__device__ __forceinline__ bool
path_line(PathArgs const &A, int line, int *x, int *y, int *len, int *extra)
{
    int const w = A.w, h = A.h;
    *extra = 0;
    if (A.dy == 0) {
        if (line >= h)
            return false;
        *y = line;
        *x = A.dx > 0 ? 0 : w - 1;
        *len = w;
    } else if (A.dx == 0) {
        if (line >= w)
            return false;
        *x = line;
        *y = A.dy > 0 ? 0 : h - 1;
        *len = h;
    } else {
        if (line >= w + h - 1)
            return false;
        int const y_entry = A.dy > 0 ? 0 : h - 1;
        int const x_entry = A.dx > 0 ? 0 : w - 1;
        if (line < w) {
            *x = line;
            *y = y_entry;
            if (*x == x_entry)
                *extra = 1;
        } else {
            int const k = line - w + 1;
            *x = x_entry;
            *y = A.dy > 0 ? k : h - 1 - k;
        }
        int const nx = A.dx > 0 ? w - *x : *x + 1;
        int const ny = A.dy > 0 ? h - *y : *y + 1;
        *len = min(nx, ny);
    }
    return true;
}

// ---- two lines per wavefront, four planes per lane, packed 16-bit arithmetic
// (round 6; DELTA form, plane counts that are multiples of four up to 128) ----
// sgm_all_paths_kernel spends ~37 vector instructions per step of a line for
// 128 planes -- two per lane, every minimum and sum a 32-bit operation, and a
// quarter of them the minimum over the wave -- and the launch is bound by
// exactly those (profiles/r6_sgm_counters.txt: 54 % issuing, 0.33 of HBM).
// Here a lane holds FOUR planes as two u16 pairs (v_pk_add_u16 / v_pk_min_u16
// work on both halves), so 32 lanes cover a line and a wave walks TWO adjacent
// lines of one direction: the step's instructions are shared by both, the
// minimum over a line is five DPP steps over a half wave instead of six over a
// whole one.  Same integers as sgm_all_paths_kernel<K, true> (every value stays
// below 2^16: L <= 255 + P2, BIG + P1 + P2 < 65536), hence the same bytes.
typedef unsigned short u16x2_r __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t
pk_add(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, (u16x2_r)(__builtin_bit_cast(u16x2_r, a)
        + __builtin_bit_cast(u16x2_r, b)));
}

__device__ __forceinline__ uint32_t
pk_sub(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, (u16x2_r)(__builtin_bit_cast(u16x2_r, a)
        - __builtin_bit_cast(u16x2_r, b)));
}

__device__ __forceinline__ uint32_t
pk_min(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(
        __builtin_bit_cast(u16x2_r, a), __builtin_bit_cast(u16x2_r, b)));
}


// FULL: 128 planes, every lane of a half wave has four (no idle lanes to reset)
//
// ADAPT: the build without SSE (sgm_stereo.cc:310-346, adapted_penalty2 above).
// penalty2' depends on |I - I'| in [0, 255] only, so the wave builds the 256
// packed values {p2', p2'} once in LDS (1 KiB, four exact integer divisions
// per lane) and a step is one broadcast ds_read_b32 indexed by the difference
// of two image bytes -- both known as soon as the bytes are loaded, which
// happens with the cost words of the chunk AHEAD, so neither the load nor the
// LDS read sits on the dependent chain of the recurrence.  (An exact division
// per step would add ~25 VALU instructions to a step of ~40.)  The image byte
// is one address per half wave: a broadcast load.
// Range of the DELTA bytes in this mode: a step stores u - min L' with
// min L' <= u <= min L' + p2' (u is a minimum of terms >= min L', one of them
// min L' + p2'), and p2' <= max(P2, P1 * 3 / 2) <= 255 by delta_form(); the
// first cell of a line stores 0, or C <= 255 at a doubly seeded corner.  The
// corner of an UPWARD diagonal sweep starts its line with L = 2 C <= 510
// (:626-654 seed the path volumes with `+=`), which changes pa / pb only: the
// byte it stores is the same C.  All 16-bit lanes stay below 2^15: L <= 510,
// BIG2 + P1 < 2^16.
template <int K, bool FULL, bool ADAPT = false>
__global__ void __launch_bounds__(64)
sgm_paths2_kernel(PathArgs A)
{
    __shared__ uint32_t p2_table[ADAPT ? 256 : 1];
    int const w = A.w, h = A.h, D = A.D;
    // block -> (direction, pair of lines), the grid being sgm_grid_line_pairs();
    // the long horizontal lines first
    int b = blockIdx.x;
    int dir = 0;
    for (; dir < 8; ++dir) {
        int const pairs_of_dir = (sgm_dir_lines(dir, w, h) + 1) >> 1;
        if (b < pairs_of_dir)
            break;
        b -= pairs_of_dir;
    }
    if (dir > 7)
        return;
    A.dx = SGM_DIRS[dir][0];
    A.dy = SGM_DIRS[dir][1];

    int const lane = threadIdx.x;
    int const half = lane >> 5, hl = lane & 31;
    if (ADAPT) {
        // entry d: |I - I'| = d (one wave per block: the barrier is a wait on LDS)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint32_t const d = (uint32_t)(lane + 64 * j);
            uint32_t const p = max(A.p1 * 3u / 2u, A.p2 / (d + 1u));
            p2_table[d] = p | (p << 16);
        }
        __syncthreads();
    }
    int x0 = 0, y0 = 0, len = 0, extra_seed = 0;
    bool const has_line = path_line(A, 2 * b + half, &x0, &y0, &len, &extra_seed);
    if (!has_line)
        len = 0;
    bool const upper = half != 0;
    bool const ok = has_line && (FULL || 4 * hl < D);
    int const li = ok ? hl : 0;
    // the line as running pointers, four planes (bytes) per lane
    size_t const o0 = has_line ? (((size_t)y0 * w + x0) * D >> 2) + li : 0;
    ptrdiff_t const step = ((ptrdiff_t)A.dy * w + A.dx) * D / 4;
    const uint32_t *__restrict__ cin = reinterpret_cast<const uint32_t *>(A.cost) + o0;
    uint32_t *__restrict__ e32
        = reinterpret_cast<uint32_t *>(A.delta + (size_t)dir * A.vol) + o0;
    // "no such plane": above every path cost, and + P1 (<= 255 in this form)
    // still fits 16 bits
    uint32_t const BIG2 = 0x7FFF7FFFu;
    uint32_t const p1p1 = (uint32_t)A.p1 | ((uint32_t)A.p1 << 16);
    uint32_t const p2p2 = (uint32_t)A.p2 | ((uint32_t)A.p2 << 16);
    // ADAPT: the image bytes of the line, one per step
    size_t const io0 = has_line ? (size_t)y0 * w + x0 : 0;
    ptrdiff_t const istep = (ptrdiff_t)A.dy * w + A.dx;
    const uint8_t *__restrict__ iin = ADAPT ? A.img + io0 : nullptr;
    uint32_t i_before = 0;
    // v_perm_b32 selectors of the two neighbour vectors that reach into the
    // adjacent lanes -- {plane 3 of the lane before, own plane 0} and {own plane
    // 3, plane 0 of the lane after} -- per lane: at the ends of a line (where
    // the lane before / after belongs to the OTHER line of the wave) the bytes
    // 0x00, 0xff instead, i.e. 0xff00: no such plane
    uint32_t const sel_below = hl == 0 ? 0x05040d0cu : 0x05040302u;   // perm(pa, pb_prev)
    uint32_t const sel_above = hl == 31 ? 0x0d0c0302u : 0x05040302u;  // perm(pa_next, pb)

    // ---- the first cell of a line: L = C (sgm_stereo.cc:457-464; a corner that
    // is seeded from its row and from its column adds C twice) ----
    uint32_t pa = BIG2, pb = BIG2;     // planes {4 hl, 4 hl + 1}, {4 hl + 2, 4 hl + 3}
    if (has_line) {
        uint32_t const c = *cin;
        uint32_t const ca = __builtin_amdgcn_perm(0u, c, 0x0c010c00u);
        uint32_t const cb = __builtin_amdgcn_perm(0u, c, 0x0c030c02u);
        if (ok) {
            pa = ca;
            pb = cb;
            if (ADAPT && extra_seed && A.dy < 0) {
                pa = pk_add(ca, ca);
                pb = pk_add(cb, cb);
            }
            *e32 = extra_seed ? c : 0u;
        }
        if (ADAPT)
            i_before = *iin;
    }
    cin += step;
    e32 += step;
    if (ADAPT)
        iin += istep;
    // the remaining steps of the two lines as scalars: every "is this step
    // inside my line" below is then a lane mask built by scalar instructions
    int const rest0 = max(__builtin_amdgcn_readlane(len, 0) - 1, 0);
    int const rest1 = max(__builtin_amdgcn_readlane(len, 32) - 1, 0);
    int const rest_max = max(rest0, rest1), rest_min = min(rest0, rest1);
    auto const inside = [&](int r) -> bool {
        return (!upper & (r < rest0)) | (upper & (r < rest1));
    };

    uint32_t c_cur[K], c_next[K], outv[K];
    uint32_t far_cur[K], far_next[K];   // ADAPT: {p2', p2'} of the steps
#pragma unroll
    for (int k = 0; k < K; ++k) {
        c_cur[k] = 0;
        if (inside(k))
            c_cur[k] = cin[(ptrdiff_t)k * step];
    }
    cin += (ptrdiff_t)K * step;
    if (ADAPT) {
        uint32_t iv[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            iv[k] = 0;
            if (inside(k))
                iv[k] = iin[(ptrdiff_t)k * istep];
        }
        iin += (ptrdiff_t)K * istep;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            uint32_t const d = iv[k] > i_before ? iv[k] - i_before : i_before - iv[k];
            far_cur[k] = p2_table[d];
            i_before = iv[k];
        }
    }
    // one chunk of K steps; FAST: this chunk and the next lie inside both lines
    // (no predicates on the loads and stores)
    auto const chunk = [&](auto fast_tag, int base) {
        constexpr bool FAST = decltype(fast_tag)::value;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            c_next[k] = 0;
            if (FAST || inside(base + K + k))
                c_next[k] = cin[(ptrdiff_t)k * step];
        }
        uint32_t iv[K];
        if (ADAPT) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                iv[k] = 0;
                if (FAST || inside(base + K + k))
                    iv[k] = iin[(ptrdiff_t)k * istep];
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            outv[k] = 0;
            if (FAST || base + k < rest_max) {
                // the four cost bytes as two u16 pairs
                uint32_t const ca = __builtin_amdgcn_perm(0u, c_cur[k], 0x0c010c00u);
                uint32_t const cb = __builtin_amdgcn_perm(0u, c_cur[k], 0x0c030c02u);
                // the minimum over the line: per lane, then over its half wave
                uint32_t m = pk_min(pa, pb);
                m = ~min(m & 0xFFFFu, m >> 16);
                m = max_dpp0<DPP_ROW_SHR1, DPP_ROWS_ALL>(m);
                m = max_dpp0<DPP_ROW_SHR2, DPP_ROWS_ALL>(m);
                m = max_dpp0<DPP_ROW_SHR4, DPP_ROWS_ALL>(m);
                m = max_dpp0<DPP_ROW_SHR8, DPP_ROWS_ALL>(m);
                m = max_dpp0<DPP_ROW_BCAST15, DPP_ROWS_1_3>(m);
                uint32_t const m_lower = ~(uint32_t)__builtin_amdgcn_readlane((int)m, 31);
                uint32_t const m_upper = ~(uint32_t)__builtin_amdgcn_readlane((int)m, 63);
                uint32_t const mm_lower = m_lower | (m_lower << 16);
                uint32_t const mm_upper = m_upper | (m_upper << 16);
                uint32_t const mnmn = upper ? mm_upper : mm_lower;
                uint32_t const far = pk_add(mnmn, ADAPT ? far_cur[k] : p2p2);
                // neighbouring planes: {3 of the lane before, 0}, {1, 2}, {3, 0 of the lane after}
                // (wave_shr:1 / wave_shl:1; the lanes without a source are ends of
                // a line, whose selectors do not look at what arrives)
                uint32_t const pb_prev = dpp_u32<DPP_WAVE_SHR1, DPP_ROWS_ALL, true>(0u, pb);
                uint32_t const pa_next = dpp_u32<DPP_WAVE_SHL1, DPP_ROWS_ALL, true>(0u, pa);
                uint32_t const below_a = __builtin_amdgcn_perm(pa, pb_prev, sel_below);
                uint32_t const mid = __builtin_amdgcn_alignbit(pb, pa, 16);
                uint32_t const above_b = __builtin_amdgcn_perm(pa_next, pb, sel_above);
                uint32_t const mid1 = pk_add(mid, p1p1);
                // :310-346: L = C + min(L'(d), L'(d -+ 1) + P1, min L' + P2) - min L'
                uint32_t const ua = pk_min(pk_min(pa, pk_add(below_a, p1p1)), pk_min(mid1, far));
                uint32_t const ub = pk_min(pk_min(pb, mid1), pk_min(pk_add(above_b, p1p1), far));
                uint32_t const ea = pk_sub(ua, mnmn), eb = pk_sub(ub, mnmn);
                pa = pk_add(ca, ea);
                pb = pk_add(cb, eb);
                outv[k] = __builtin_amdgcn_perm(eb, ea, 0x06040200u);
                if (!FULL && !ok)
                    pa = pb = BIG2;
            }
        }
        if (ADAPT) {
            // the penalties of the chunk ahead (a step past the end of a line
            // reads image byte 0: an entry of the table like any other, and what
            // that step computes is never stored)
#pragma unroll
            for (int k = 0; k < K; ++k) {
                uint32_t const d = iv[k] > i_before ? iv[k] - i_before : i_before - iv[k];
                far_next[k] = p2_table[d];
                i_before = iv[k];
            }
        }
        if (FULL && FAST) {
#pragma unroll
            for (int k = 0; k < K; ++k)
                e32[(ptrdiff_t)k * step] = outv[k];
        } else if (ok) {
#pragma unroll
            for (int k = 0; k < K; ++k)
                if (FAST || inside(base + k))
                    e32[(ptrdiff_t)k * step] = outv[k];
        }
    };
    for (int base = 0; base < rest_max; base += K) {
        if (base + 2 * K <= rest_min)
            chunk(std::true_type(), base);
        else
            chunk(std::false_type(), base);
        cin += (ptrdiff_t)K * step;
        e32 += (ptrdiff_t)K * step;
#pragma unroll
        for (int k = 0; k < K; ++k)
            c_cur[k] = c_next[k];
        if (ADAPT) {
            iin += (ptrdiff_t)K * istep;
#pragma unroll
            for (int k = 0; k < K; ++k)
                far_cur[k] = far_next[k];
        }
    }
}

// All eight path directions in ONE launch.  The recurrences of different
// directions are independent; only their sums meet in S.  Since the sums are
// wrapping integer adds, S is accumulated with device-scope atomic adds on
// the packed u32 (two u16 planes that cannot carry into each other: eight
// paths of at most 255 + P2 plus the seeds stay below 65536), so the result
// is bit-exact for any interleaving.  ~9000 wavefronts instead of <= 1500 per
// launch, and the wall time is the longest line instead of the sum over
// directions.  S must be zeroed first.
//
// DELTA form (penalty2 <= 255): what a path adds to S at a pixel is
// L = C + (u - min_prev) with 0 <= u - min_prev <= P2 (sgm_stereo.cc:310-346:
// u is the minimum of terms that are all >= min_prev, one of them min_prev +
// P2), and C -- or 2 C at a doubly seeded corner -- at the start of a line.
// So every direction stores L - C as ONE BYTE per cell into its own volume
// with plain coalesced stores (each cell lies on exactly one line per
// direction: no atomics, no zero fill) and sgm_sum_wta_kernel forms
// S = 8 C + the eight bytes on the fly: 16 + 9 bytes per cost cell instead of
// 8 x (1 + 4) + 2 with the read-modify-writes of the u16 volume.
//
// ADAPT (the build without SSE): penalty2 per step from the image byte of the
// step and of the step before (adapted_penalty2: an exact integer division on
// values that are uniform over the wave and known a chunk ahead of the
// recurrence; this kernel serves penalty2 > 255 too, which a byte-indexed
// table of packed u16 pairs would serve as well, but the division is off the
// dependent chain here and keeps the fall-back free of LDS).  The corner of an
// upward diagonal sweep starts with L = 2 C (:626-654).  DELTA bytes: as in
// sgm_paths2_kernel, u - min L' <= p2' <= 255.  Without DELTA a path adds at
// most max(510, 255 + p2') to a u16 of S (check_sgm_options).
template <int K, bool DELTA, bool ADAPT = false>
__global__ void __launch_bounds__(64)
sgm_all_paths_kernel(PathArgs A)
{
    // block -> (direction, line), the grid being sgm_grid_lines(); the long
    // horizontal lines come first.  (The two horizontal directions by a
    // division, the rest by a walk: sgm_paths2_kernel's single walk over all
    // eight compiles to other instructions here, so this decode keeps its form
    // and takes only its counts from sgm_dir_lines().)
    int const w = A.w, h = A.h, D = A.D;
    int const rows = sgm_dir_lines(0, w, h);   // == sgm_dir_lines(1, w, h)
    int b = blockIdx.x;
    int dir;
    if (b < 2 * rows) {
        dir = b / rows;           // 0: ->, 1: <-
        b -= dir * rows;
    } else {
        b -= 2 * rows;
        // remaining six: (0,1) (1,1) (-1,1) (0,-1) (1,-1) (-1,-1)
        dir = 2;
        for (int k = 2; k < 8; ++k) {
            int const lines_of_dir = sgm_dir_lines(k, w, h);
            if (b < lines_of_dir)
                break;
            b -= lines_of_dir;
            dir += 1;
        }
        if (dir > 7)
            return;
    }
    A.dx = SGM_DIRS[dir][0];
    A.dy = SGM_DIRS[dir][1];

    int const lane = threadIdx.x;
    int x0, y0, len, extra_seed;
    if (!path_line(A, b, &x0, &y0, &len, &extra_seed))
        return;
    int const pairs = D >> 1;
    bool const ok = lane < pairs;
    int const li = ok ? lane : 0;
    // The line as two running pointers (cost in, path bytes / S out): the
    // cell of step s is `step` u16 pairs behind the cell of step s - 1.
    size_t const o0 = (((size_t)y0 * w + x0) * D >> 1) + li;
    ptrdiff_t const step = ((ptrdiff_t)A.dy * w + A.dx) * D / 2;
    const uint16_t *__restrict__ cin = reinterpret_cast<const uint16_t *>(A.cost) + o0;
    uint32_t *__restrict__ s32 = reinterpret_cast<uint32_t *>(A.sgm) + o0;
    uint16_t *__restrict__ e16
        = reinterpret_cast<uint16_t *>(A.delta + (size_t)dir * A.vol) + o0;
    // "no such plane" / "lane without planes": above every path cost
    // (L <= 255 + P2 < 2^15 by check_sgm_options), and BIG + P1 still fits 16
    // bits, so no sum below needs a mask
    uint32_t const BIG = 0x7FFFu;
    uint32_t prev0 = BIG, prev1 = BIG;
    // ADAPT: the image bytes of the line, one per step
    ptrdiff_t const istep = (ptrdiff_t)A.dy * w + A.dx;
    const uint8_t *__restrict__ iin = ADAPT ? A.img + ((size_t)y0 * w + x0) : nullptr;
    uint32_t i_before = 0;

    uint32_t c_cur[K], c_next[K], addv[K];
    uint32_t p2_cur[K], p2_next[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        c_cur[k] = 0;
        if (k < len)
            c_cur[k] = cin[(ptrdiff_t)k * step];
        if (ADAPT) {
            uint32_t const i_here = k < len ? iin[(ptrdiff_t)k * istep] : 0u;
            p2_cur[k] = adapted_penalty2(A.p1, A.p2, i_here, i_before);
            i_before = i_here;
        }
    }
    cin += (ptrdiff_t)K * step;
    if (ADAPT)
        iin += (ptrdiff_t)K * istep;
    for (int base = 0; base < len; base += K) {
        int const n = min(K, len - base);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            c_next[k] = 0;
            if (base + K + k < len)
                c_next[k] = cin[(ptrdiff_t)k * step];
            if (ADAPT) {
                uint32_t const i_here = base + K + k < len ? iin[(ptrdiff_t)k * istep] : 0u;
                p2_next[k] = adapted_penalty2(A.p1, A.p2, i_here, i_before);
                i_before = i_here;
            }
        }
        cin += (ptrdiff_t)K * step;
        if (ADAPT)
            iin += (ptrdiff_t)K * istep;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            addv[k] = 0;
            if (k < n) {
                int const s = base + k;
                uint32_t const c0 = c_cur[k] & 0xFFu, c1 = c_cur[k] >> 8;
                uint32_t e0, e1;     // what the path adds beyond C
                if (s == 0) {
                    // sgm_stereo.cc:457-464: the line starts with L = C; a corner
                    // that is seeded from its row and from its column adds C twice
                    e0 = extra_seed ? c0 : 0u;
                    e1 = extra_seed ? c1 : 0u;
                    prev0 = c0;
                    prev1 = c1;
                    if (ADAPT && extra_seed && A.dy < 0) {
                        prev0 = 2u * c0;
                        prev1 = 2u * c1;
                    }
                } else {
                    // :310-346: L = C + min(L'(d), L'(d -+ 1) + P1, min L' + P2) - min L'
                    uint32_t const mn = wave_min_u32(min(prev0, prev1));
                    uint32_t const left = lane_prev(prev1, BIG);
                    uint32_t const right = lane_next(prev0, BIG);
                    uint32_t const far = mn + (ADAPT ? p2_cur[k] : A.p2);
                    uint32_t const u0 = min(min(prev0, left + A.p1), min(prev1 + A.p1, far));
                    uint32_t const u1 = min(min(prev1, prev0 + A.p1), min(right + A.p1, far));
                    e0 = u0 - mn;
                    e1 = u1 - mn;
                    prev0 = c0 + e0;
                    prev1 = c1 + e1;
                }
                if (DELTA)
                    addv[k] = e0 | (e1 << 8);
                else
                    addv[k] = (c0 + e0) | ((c1 + e1) << 16);
                if (!ok)
                    prev0 = prev1 = BIG;
            }
        }
        if (ok) {
#pragma unroll
            for (int k = 0; k < K; ++k)
                if (k < n) {
                    if (DELTA)
                        e16[(ptrdiff_t)k * step] = (uint16_t)addv[k];
                    else
                        (void)__hip_atomic_fetch_add(&s32[(ptrdiff_t)k * step], addv[k],
                            __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
        }
        e16 += (ptrdiff_t)K * step;
        s32 += (ptrdiff_t)K * step;
#pragma unroll
        for (int k = 0; k < K; ++k)
            c_cur[k] = c_next[k];
        if (ADAPT) {
#pragma unroll
            for (int k = 0; k < K; ++k)
                p2_cur[k] = p2_next[k];
        }
    }
}

// ---- one line per wavefront, four planes per lane, packed 16-bit arithmetic:
// the plane counts above 128 (multiples of four up to SGM_MAX_PLANES = 256;
// check_sgm_plane_count admits the multiples of eight) ----
// sgm_paths2_kernel's step on a whole wave: lane l holds planes 4 l .. 4 l + 3 as
// two u16 pairs, 64 lanes cover up to 256 planes, the cost words of the chunk
// ahead are loaded before the recurrence of the current chunk starts.  What
// differs from the half-wave kernel is what crosses lanes:
//   * the neighbouring planes come from lane -+ 1 of the WAVE (wave_shr:1 /
//     wave_shl:1 cross the rows and the 32-lane boundary); only lane 0 and, in
//     FULL, lane 63 have no source;
//   * the minimum of a line runs over 64 lanes (wave_max_dpp0 of the
//     complements: four row shifts, row_bcast:15, row_bcast:31, one readlane).
// A step's instructions serve ONE line here, not two.
//
// FULL: 256 planes, every lane has four (no idle lanes to reset).
// ADAPT: penalty2' from the 256-entry LDS table of packed {p2', p2'}, read for
// the chunk ahead (sgm_paths2_kernel's comment).
// DELTA (largest penalty2 <= 255): L - C as one byte per cell into the
// direction's own volume, plain stores.  Without DELTA the lane adds its two
// u16 pairs {L, L} into S with two u32 atomics (sgm_all_paths_kernel's
// argument: no 16-bit half of S carries, check_sgm_penalties).
//
// Same integers as sgm_all_paths_kernel, hence the same bytes.  Range, with
// Pmax = the largest penalty2 of a step (<= 255 with DELTA, <= 7808 without, by
// check_sgm_penalties): a line starts with L = C <= 255, or 2 C <= 510 at the
// doubly seeded corner of an upward diagonal in ADAPT; a step gives
// L = C + u - min L' with min L' <= u <= min L' + p2', so L <= 255 + Pmax
// behind the start and every sum of a step is <= max(510, 255 + Pmax) + Pmax
// < 2^15.  The sentinel BIG2 = 0x7FFF per half is above every L, and
// BIG2 + P1 <= 0x7FFF + 7808 < 2^16 (P1 <= Pmax in both modes).  The DELTA
// form marks a missing neighbour plane at the ends of the line with 0xFF00 out
// of the byte permute: 0xFF00 + P1 <= 0xFFFF since P1 <= 255 there; without
// DELTA the lane without a source keeps BIG2 as the DPP move's old value.
// Bytes stored with DELTA: u - min L' <= p2' <= 255; C at a doubly seeded corner.
template <int K, bool FULL, bool ADAPT, bool DELTA>
__global__ void __launch_bounds__(64)
sgm_paths_wide_kernel(PathArgs A)
{
    __shared__ uint32_t p2_table[ADAPT ? 256 : 1];
    int const w = A.w, h = A.h, D = A.D;
    // block -> (direction, line), the grid being sgm_grid_lines(); the long
    // horizontal lines first
    int b = blockIdx.x;
    int dir = 0;
    for (; dir < 8; ++dir) {
        int const lines_of_dir = sgm_dir_lines(dir, w, h);
        if (b < lines_of_dir)
            break;
        b -= lines_of_dir;
    }
    if (dir > 7)
        return;
    A.dx = SGM_DIRS[dir][0];
    A.dy = SGM_DIRS[dir][1];

    int const lane = threadIdx.x;
    if (ADAPT) {
        // entry d: |I - I'| = d (one wave per block: the barrier is a wait on LDS)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint32_t const d = (uint32_t)(lane + 64 * j);
            uint32_t const p = max(A.p1 * 3u / 2u, A.p2 / (d + 1u));
            p2_table[d] = p | (p << 16);
        }
        __syncthreads();
    }
    int x0 = 0, y0 = 0, len = 0, extra_seed = 0;
    if (!path_line(A, b, &x0, &y0, &len, &extra_seed))
        return;
    bool const ok = FULL || 4 * lane < D;
    int const li = ok ? lane : 0;
    // the line as running pointers, four planes (bytes) per lane
    size_t const o0 = (((size_t)y0 * w + x0) * D >> 2) + li;
    ptrdiff_t const step = ((ptrdiff_t)A.dy * w + A.dx) * D / 4;
    const uint32_t *__restrict__ cin = reinterpret_cast<const uint32_t *>(A.cost) + o0;
    uint32_t *__restrict__ e32
        = reinterpret_cast<uint32_t *>(A.delta + (DELTA ? (size_t)dir * A.vol : 0)) + o0;
    // without DELTA: the lane's two u16 pairs of S
    uint32_t *__restrict__ s32 = reinterpret_cast<uint32_t *>(A.sgm) + 2 * o0;
    uint32_t const BIG2 = 0x7FFF7FFFu;
    uint32_t const p1p1 = (uint32_t)A.p1 | ((uint32_t)A.p1 << 16);
    uint32_t const p2p2 = (uint32_t)A.p2 | ((uint32_t)A.p2 << 16);
    // ADAPT: the image bytes of the line, one per step
    ptrdiff_t const istep = (ptrdiff_t)A.dy * w + A.dx;
    const uint8_t *__restrict__ iin = ADAPT ? A.img + ((size_t)y0 * w + x0) : nullptr;
    uint32_t i_before = 0;
    // DELTA: v_perm_b32 selectors of the two neighbour vectors that reach into
    // the adjacent lanes -- {plane 3 of the lane before, own plane 0} and {own
    // plane 3, plane 0 of the lane after}; lane 0 and lane 63 have no such lane
    // and take the bytes 0x00, 0xff instead, i.e. 0xff00: no such plane.  (An
    // idle lane after the last one of the line holds BIG2: no selector needed.)
    uint32_t const sel_below = DELTA && lane == 0 ? 0x05040d0cu : 0x05040302u;   // perm(pa, pb_prev)
    uint32_t const sel_above = DELTA && lane == 63 ? 0x0d0c0302u : 0x05040302u;  // perm(pa_next, pb)

    // ---- the first cell of the line: L = C (sgm_stereo.cc:457-464; a corner
    // that is seeded from its row and from its column adds C twice) ----
    uint32_t pa = BIG2, pb = BIG2;     // planes {4 l, 4 l + 1}, {4 l + 2, 4 l + 3}
    {
        uint32_t const c = *cin;
        uint32_t const ca = __builtin_amdgcn_perm(0u, c, 0x0c010c00u);
        uint32_t const cb = __builtin_amdgcn_perm(0u, c, 0x0c030c02u);
        if (ok) {
            pa = ca;
            pb = cb;
            if (ADAPT && extra_seed && A.dy < 0) {
                pa = pk_add(ca, ca);
                pb = pk_add(cb, cb);
            }
            if (DELTA) {
                *e32 = extra_seed ? c : 0u;
            } else {
                (void)__hip_atomic_fetch_add(s32, extra_seed ? pk_add(ca, ca) : ca,
                    __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                (void)__hip_atomic_fetch_add(s32 + 1, extra_seed ? pk_add(cb, cb) : cb,
                    __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        if (ADAPT)
            i_before = *iin;
    }
    cin += step;
    e32 += step;
    s32 += 2 * step;
    if (ADAPT)
        iin += istep;
    // the remaining steps of the line, a scalar
    int const rest = max(__builtin_amdgcn_readfirstlane(len) - 1, 0);

    uint32_t c_cur[K], c_next[K], outa[K], outb[K];
    uint32_t far_cur[K], far_next[K];   // ADAPT: {p2', p2'} of the steps
#pragma unroll
    for (int k = 0; k < K; ++k) {
        c_cur[k] = 0;
        if (k < rest)
            c_cur[k] = cin[(ptrdiff_t)k * step];
    }
    cin += (ptrdiff_t)K * step;
    if (ADAPT) {
        uint32_t iv[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            iv[k] = 0;
            if (k < rest)
                iv[k] = iin[(ptrdiff_t)k * istep];
        }
        iin += (ptrdiff_t)K * istep;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            uint32_t const d = iv[k] > i_before ? iv[k] - i_before : i_before - iv[k];
            far_cur[k] = p2_table[d];
            i_before = iv[k];
        }
    }
    // one chunk of K steps; FAST: this chunk and the next lie inside the line
    // (no predicates on the loads and stores)
    auto const chunk = [&](auto fast_tag, int base) {
        constexpr bool FAST = decltype(fast_tag)::value;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            c_next[k] = 0;
            if (FAST || base + K + k < rest)
                c_next[k] = cin[(ptrdiff_t)k * step];
        }
        uint32_t iv[K];
        if (ADAPT) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                iv[k] = 0;
                if (FAST || base + K + k < rest)
                    iv[k] = iin[(ptrdiff_t)k * istep];
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            outa[k] = outb[k] = 0;
            if (FAST || base + k < rest) {
                // the four cost bytes as two u16 pairs
                uint32_t const ca = __builtin_amdgcn_perm(0u, c_cur[k], 0x0c010c00u);
                uint32_t const cb = __builtin_amdgcn_perm(0u, c_cur[k], 0x0c030c02u);
                // the minimum over the line: per lane, then over the wave
                uint32_t m = pk_min(pa, pb);
                m = wave_max_dpp0(~min(m & 0xFFFFu, m >> 16));
                uint32_t const mn = ~m;
                uint32_t const mnmn = mn | (mn << 16);
                uint32_t const far = pk_add(mnmn, ADAPT ? far_cur[k] : p2p2);
                // neighbouring planes: {3 of the lane before, 0}, {1, 2}, {3, 0 of the lane after}
                uint32_t pb_prev, pa_next;
                if (DELTA) {
                    // (a lane without a source reads 0; its selector does not
                    // look at what arrives)
                    pb_prev = dpp_u32<DPP_WAVE_SHR1, DPP_ROWS_ALL, true>(0u, pb);
                    pa_next = dpp_u32<DPP_WAVE_SHL1, DPP_ROWS_ALL, true>(0u, pa);
                } else {
                    pb_prev = lane_prev(pb, BIG2);
                    pa_next = lane_next(pa, BIG2);
                }
                uint32_t const below_a = __builtin_amdgcn_perm(pa, pb_prev, sel_below);
                uint32_t const mid = __builtin_amdgcn_alignbit(pb, pa, 16);
                uint32_t const above_b = __builtin_amdgcn_perm(pa_next, pb, sel_above);
                uint32_t const mid1 = pk_add(mid, p1p1);
                // :310-346: L = C + min(L'(d), L'(d -+ 1) + P1, min L' + P2) - min L'
                uint32_t const ua = pk_min(pk_min(pa, pk_add(below_a, p1p1)), pk_min(mid1, far));
                uint32_t const ub = pk_min(pk_min(pb, mid1), pk_min(pk_add(above_b, p1p1), far));
                uint32_t const ea = pk_sub(ua, mnmn), eb = pk_sub(ub, mnmn);
                pa = pk_add(ca, ea);
                pb = pk_add(cb, eb);
                if (DELTA) {
                    outa[k] = __builtin_amdgcn_perm(eb, ea, 0x06040200u);
                } else {
                    outa[k] = pa;
                    outb[k] = pb;
                }
                if (!FULL && !ok)
                    pa = pb = BIG2;
            }
        }
        if (ADAPT) {
            // the penalties of the chunk ahead (a step past the end of the line
            // reads image byte 0: an entry of the table like any other, and what
            // that step computes is never stored)
#pragma unroll
            for (int k = 0; k < K; ++k) {
                uint32_t const d = iv[k] > i_before ? iv[k] - i_before : i_before - iv[k];
                far_next[k] = p2_table[d];
                i_before = iv[k];
            }
        }
        if (FULL || ok) {
#pragma unroll
            for (int k = 0; k < K; ++k)
                if (FAST || base + k < rest) {
                    if (DELTA) {
                        e32[(ptrdiff_t)k * step] = outa[k];
                    } else {
                        (void)__hip_atomic_fetch_add(&s32[2 * (ptrdiff_t)k * step], outa[k],
                            __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        (void)__hip_atomic_fetch_add(&s32[2 * (ptrdiff_t)k * step + 1], outb[k],
                            __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                }
        }
    };
    for (int base = 0; base < rest; base += K) {
        if (base + 2 * K <= rest)
            chunk(std::true_type(), base);
        else
            chunk(std::false_type(), base);
        cin += (ptrdiff_t)K * step;
        e32 += (ptrdiff_t)K * step;
        s32 += 2 * (ptrdiff_t)K * step;
#pragma unroll
        for (int k = 0; k < K; ++k)
            c_cur[k] = c_next[k];
        if (ADAPT) {
            iin += (ptrdiff_t)K * istep;
#pragma unroll
            for (int k = 0; k < K; ++k)
                far_cur[k] = far_next[k];
        }
    }
}

// The end of both WTA kernels (sgm_stereo.cc:300-303): the winning plane is the
// low byte of the (value, plane) key; no depth for the two nearest planes and
// for dark pixels.
__device__ __forceinline__ void
wta_store(uint32_t key, size_t p, const uint8_t *__restrict__ main_img,
    const float *__restrict__ depths, float *__restrict__ depth,
    int32_t *__restrict__ argmin)
{
    int const min_index = (int)(key & 0xFFu);
    if (argmin != nullptr)
        argmin[p] = min_index;
    if (depth != nullptr)
        depth[p] = (min_index < 2 || main_img[p] < 25) ? 0.0f
            : depths[min_index];
}

// WTA with 16 lanes per pixel (sgm_stereo.cc:274-306): lane sub reads planes
// sub, sub + 16, ...; the first minimum wins through the (value, plane) key.
__global__ void __launch_bounds__(256)
wta_rows_kernel(const uint16_t *__restrict__ sgm,
    const uint8_t *__restrict__ main_img, const float *__restrict__ depths,
    size_t npix, int D, float *__restrict__ depth, int32_t *__restrict__ argmin)
{
    size_t const p = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    int const sub = threadIdx.x & 15;
    uint32_t key = 0xFFFFFFFFu;
    if (p < npix)
        for (int d = sub; d < D; d += 16)
            key = min(key, (uint32_t)sgm[p * D + d] * 256u + (uint32_t)d);
    key = row_prefix_min_u32(key);
    if (sub == 15 && p < npix)
        wta_store(key, p, main_img, depths, depth, argmin);
}

// S = 8 C + the eight path bytes of the DELTA form, and the winner-takes-all of
// wta_rows_kernel on it, 32 lanes per pixel with four planes each (one u32
// per volume and lane).  S itself is only written when the caller wants the
// volume (smvs_sgm_run's `sgm` output).
__global__ void __launch_bounds__(256)
sgm_sum_wta_kernel(const uint8_t *__restrict__ cost, const uint8_t *__restrict__ delta,
    size_t vol, const uint8_t *__restrict__ main_img, const float *__restrict__ depths,
    size_t npix, int D, float *__restrict__ depth, int32_t *__restrict__ argmin,
    uint16_t *__restrict__ sgm_out)
{
    size_t const p = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 5;
    int const sub = threadIdx.x & 31;
    int const d0 = 4 * sub;
    uint32_t key = 0xFFFFFFFFu;
    if (p < npix && d0 < D) {
        size_t const o = p * (size_t)D + d0;   // D % 4 == 0: aligned u32
        uint32_t const c = *reinterpret_cast<const uint32_t *>(cost + o);
        uint32_t e[8];
#pragma unroll
        for (int k = 0; k < 8; ++k)
            e[k] = *reinterpret_cast<const uint32_t *>(delta + (size_t)k * vol + o);
        uint32_t sv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint32_t sum = 8u * ((c >> (8 * j)) & 0xFFu);
#pragma unroll
            for (int k = 0; k < 8; ++k)
                sum += (e[k] >> (8 * j)) & 0xFFu;
            sv[j] = sum & 0xFFFFu;
            key = min(key, sv[j] * 256u + (uint32_t)(d0 + j));
        }
        if (sgm_out != nullptr) {
            uint2 const packed = make_uint2(sv[0] | (sv[1] << 16), sv[2] | (sv[3] << 16));
            *reinterpret_cast<uint2 *>(sgm_out + o) = packed;
        }
    }
    // minimum over the 32 lanes of the pixel: inside the rows of 16 by DPP
    // shifts, then across the two rows
    key = row_prefix_min_u32(key);
    // lanes 15 and 31 of the pixel hold the row minima
    uint32_t const other = (uint32_t)__shfl_xor((int)key, 16);
    key = min(key, other);
    if (sub == 31 && p < npix)
        wta_store(key, p, main_img, depths, depth, argmin);
}

// The same with 64 lanes per pixel, for the plane counts above 128: a wavefront
// is one pixel, so the minimum over the four rows of 16 lanes is the wave's
// (row_prefix_min_u32, then row_bcast:15 / row_bcast:31 -- wave_min_u32).  The
// plane index uses the key's whole low byte at 256 planes; S < 2^16 keeps
// value * 256 + plane inside 32 bits.
__global__ void __launch_bounds__(256)
sgm_sum_wta_wide_kernel(const uint8_t *__restrict__ cost, const uint8_t *__restrict__ delta,
    size_t vol, const uint8_t *__restrict__ main_img, const float *__restrict__ depths,
    size_t npix, int D, float *__restrict__ depth, int32_t *__restrict__ argmin,
    uint16_t *__restrict__ sgm_out)
{
    size_t const p = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    int const sub = threadIdx.x & 63;
    int const d0 = 4 * sub;
    uint32_t key = 0xFFFFFFFFu;
    if (p < npix && d0 < D) {
        size_t const o = p * (size_t)D + d0;   // D % 4 == 0: aligned u32
        uint32_t const c = *reinterpret_cast<const uint32_t *>(cost + o);
        uint32_t e[8];
#pragma unroll
        for (int k = 0; k < 8; ++k)
            e[k] = *reinterpret_cast<const uint32_t *>(delta + (size_t)k * vol + o);
        uint32_t sv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint32_t sum = 8u * ((c >> (8 * j)) & 0xFFu);
#pragma unroll
            for (int k = 0; k < 8; ++k)
                sum += (e[k] >> (8 * j)) & 0xFFu;
            sv[j] = sum & 0xFFFFu;
            key = min(key, sv[j] * 256u + (uint32_t)(d0 + j));
        }
        if (sgm_out != nullptr) {
            uint2 const packed = make_uint2(sv[0] | (sv[1] << 16), sv[2] | (sv[3] << 16));
            *reinterpret_cast<uint2 *>(sgm_out + o) = packed;
        }
    }
    key = wave_min_u32(key);
    if (sub == 63 && p < npix)
        wta_store(key, p, main_img, depths, depth, argmin);
}

__global__ void __launch_bounds__(256)
widen_u8_kernel(const uint8_t *__restrict__ src, uint16_t *__restrict__ dst,
    size_t n)
{
    size_t const i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        dst[i] = src[i];
}

// The counters of the optional per-kernel event timer (SgmProfile,
// sgm_internal.h; smvs_sgm_profile below): one copy for the whole library, the
// launches of sgm_view.hip and bilateral.hip report here too.
std::mutex g_sgm_prof_mutex;
bool g_sgm_prof_on = false;
double g_sgm_prof_ms[SMVS_SGM_K_COUNT] = { 0 };
long long g_sgm_prof_launches[SMVS_SGM_K_COUNT] = { 0 };

SgmProfile::SgmProfile()
{
    std::lock_guard<std::mutex> guard(g_sgm_prof_mutex);
    on = g_sgm_prof_on;
}

SgmProfile::~SgmProfile()
{
    if (pending.empty())
        return;
    std::lock_guard<std::mutex> guard(g_sgm_prof_mutex);
    for (auto &p : pending) {
        float ms = 0.f;
        if (hipEventSynchronize(p.b) == hipSuccess
            && hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            g_sgm_prof_ms[p.cls] += ms;
            g_sgm_prof_launches[p.cls] += 1;
        }
        (void)hipEventDestroy(p.a);
        (void)hipEventDestroy(p.b);
    }
}

// (declared in sgm_internal.h)
int
check_sgm_penalties(unsigned penalty1, unsigned penalty2, int p2_mode)
{
    SMVS_REQUIRE(p2_mode == SMVS_SGM_P2_CONSTANT || p2_mode == SMVS_SGM_P2_ADAPTIVE,
        "unknown penalty2 mode");
    // The all-paths kernel adds the eight path costs into S with u32 atomics
    // on packed u16 pairs: exact only while no 16-bit lane can carry into its
    // neighbour, i.e. while S stays below 2^16.  Per path L <= 255 + P2 (Q20),
    // border pixels add C up to 4 times more (Q19).  The reference wraps every
    // u16 lane on its own (_mm_add_epi16), which this bound never reaches.
    //
    // SMVS_SGM_P2_ADAPTIVE (the build without SSE, sgm_stereo.cc:310-346), the
    // same bound re-derived: a step uses p2' = max(P1 * 3 / 2, P2 / diff), so
    // p2' <= Pmax = max(P2, P1 * 3 / 2).  A line starts with L = C <= 255, or
    // with 2 C <= 510 at the corner of an upward diagonal sweep (:626-654 seed
    // the path volumes with `+=`); a step gives L = C + u - min L' with
    // min L' <= u <= min L' + p2', hence L <= 255 + Pmax behind the start
    // whatever the start held.  What a line adds to S at its start is its seed
    // (C, twice at a corner) -- the same "up to 4 C more" (Q19) -- so
    // S <= 8 (255 + Pmax) + 4 * 255.  Inside the bound no sum of the
    // reference's literal loop wraps either (L' + p2' <= max(510, 255 + Pmax)
    // + Pmax), so its uint16_t narrowing never acts.
    // penalty2 < penalty1 is ACCEPTED in this mode: p2' >= P1 * 3 / 2 >= P1 at
    // every step, which is all the recurrence (and its closed form) needs; the
    // constant mode keeps refusing it.
    if (p2_mode == SMVS_SGM_P2_CONSTANT)
        SMVS_REQUIRE(penalty2 >= penalty1, "penalty2 must not be below penalty1");
    unsigned const pmax = SgmWorkspace::largest_penalty2(penalty1, penalty2, p2_mode);
    SMVS_REQUIRE(penalty1 <= 0xFFFFu && penalty2 <= 0xFFFFu
            && 8u * (255u + pmax) + 4u * 255u < 65536u,
        "penalty2 too large for the u16 aggregation volume");
    return SMVS_OK;
}

// (declared in sgm_internal.h)
int
check_sgm_plane_count(int num_steps)
{
    SMVS_REQUIRE(sgm_plane_count_ok(num_steps),
        "num_steps must be in [2, 128] or a multiple of 8 in [136, 256]");
    return SMVS_OK;
}

static int
check_sgm_options(int num_steps, float min_depth, float max_depth,
    unsigned penalty1, unsigned penalty2, int p2_mode = SMVS_SGM_P2_CONSTANT)
{
    SMVS_REQUIRE(p2_mode == SMVS_SGM_P2_CONSTANT || p2_mode == SMVS_SGM_P2_ADAPTIVE,
        "unknown penalty2 mode");
    int const rc = check_sgm_plane_count(num_steps);
    if (rc != SMVS_OK)
        return rc;
    SMVS_REQUIRE(min_depth > 0.f && max_depth > min_depth, "bad depth range");
    return check_sgm_penalties(penalty1, penalty2, p2_mode);
}

// (declared in sgm_internal.h)
int
sgm_run_device(SgmWorkspace &B, const uint8_t *d_main,
    int w, int h, const uint8_t *d_nbr, int nw, int nh, const float *M,
    const float *t, float min_depth, float max_depth, int num_steps,
    uint16_t penalty1, uint16_t penalty2, int p2_mode, float *d_depth)
{
    int rc = check_sgm_options(num_steps, min_depth, max_depth, penalty1,
        penalty2, p2_mode);
    if (rc != SMVS_OK)
        return rc;
    SMVS_REQUIRE(B.runs < SgmWorkspace::MAX_RUNS, "too many runs on one workspace");
    hipStream_t const stream = B.ws->stream;
    size_t const npix = (size_t)w * h;
    size_t const vol = npix * num_steps;
    bool const adapt = p2_mode == SMVS_SGM_P2_ADAPTIVE;
    // (what decides the form of the volumes: the largest penalty2 of a step)
    unsigned const pmax = SgmWorkspace::largest_penalty2(penalty1, penalty2, p2_mode);
    if ((rc = B.ensure(npix, num_steps, pmax)) != SMVS_OK)
        return rc;
    // sgm_stereo.cc:195-203: inverse-depth planes by repeated float addition
    float depths[SGM_MAX_PLANES];
    {
#pragma clang fp contract(off)
        float inv_depth = 1.0f / max_depth;
        float const increment = (1.0f / min_depth - inv_depth) / (num_steps - 1);
        for (int i = 0; i < num_steps; ++i) {
            depths[i] = 1.0f / inv_depth;
            inv_depth += increment;
        }
    }
    float *d_depths = B.depths + SGM_MAX_PLANES * B.runs;
    B.runs += 1;
    if ((rc = B.ws->upload(d_depths, depths, sizeof(float) * num_steps)) != SMVS_OK)
        return rc;

    {
        SgmKernelTimer timer(B.prof, stream, SMVS_SGM_K_CENSUS);
        hipLaunchKernelGGL(census_main_kernel, dim3((w + 255) / 256, h), dim3(256),
            0, stream, d_main, w, h, B.census);
    }
    WarpArgs W;
    W.neighbor = d_nbr;
    W.nw = nw;
    W.nh = nh;
    memcpy(W.M, M, sizeof(float) * 9);
    memcpy(W.t, t, sizeof(float) * 3);
    W.depths = d_depths;
    W.D = num_steps;
    W.w = w;
    W.h = h;
    W.warped = B.warped;
    {
        SgmKernelTimer timer(B.prof, stream, SMVS_SGM_K_WARP);
        hipLaunchKernelGGL(warp_kernel, dim3((unsigned)((w + WARP_TILE - 1) / WARP_TILE),
            (unsigned)h, (unsigned)((num_steps + WARP_TILE - 1) / WARP_TILE)),
            dim3(WARP_TILE), 0, stream, W);
    }
    {
        SgmKernelTimer timer(B.prof, stream, SMVS_SGM_K_COST);
        int const tiles = ((w + CT_W - 1) / CT_W) * ((h + CT_H - 1) / CT_H);
        // (the packed kernel stages four planes per load; any other plane count
        // takes the one-plane-per-lane kernel)
        if ((num_steps & 3) == 0)
            hipLaunchKernelGGL(cost_packed_kernel,
                dim3(((tiles + 7) / 8) * 8, (num_steps + CP_D - 1) / CP_D),
                dim3(256), 0, stream, B.warped, B.census, w, h, num_steps, B.cost);
        else
            hipLaunchKernelGGL(cost_tiled_kernel,
                dim3(tiles, (num_steps + CT_D - 1) / CT_D), dim3(256), 0, stream,
                B.warped, B.census, w, h,
                num_steps, B.cost);
    }
    SMVS_HIP_CHECK(hipGetLastError());

    PathArgs P;
    P.cost = B.cost;
    P.sgm = B.sgm;
    P.w = w;
    P.h = h;
    P.D = num_steps;
    P.p1 = penalty1;
    P.p2 = penalty2;
    P.last = 0;
    P.delta = B.delta;
    P.vol = vol;
    P.img = d_main;
    bool const df = SgmWorkspace::delta_form(num_steps, pmax);
    // (SMVS_SGM_PATHS=wave: a wave per line, two planes per lane -- rounds 3-5)
    static bool const wave_per_line = [] {
        const char *e = std::getenv("SMVS_SGM_PATHS");
        return e != nullptr && e[0] == 'w';
    }();
    if (num_steps > 128) {
        // a line per wave, four planes per lane (multiples of 8 up to
        // SGM_MAX_PLANES: check_sgm_plane_count); S zeroed for the atomics
        if (!df)
            SMVS_HIP_CHECK(hipMemsetAsync(B.sgm, 0, sizeof(uint16_t) * vol, stream));
        P.dx = P.dy = 0;
        P.first = 0;
        int const lines = sgm_grid_lines(w, h);
        bool const full = num_steps == SGM_MAX_PLANES;
        SgmKernelTimer timer(B.prof, stream, SMVS_SGM_K_PATHS);
        auto const launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(lines), dim3(64), 0, stream, P);
        };
        if (df) {
            if (adapt)
                full ? launch(sgm_paths_wide_kernel<8, true, true, true>)
                     : launch(sgm_paths_wide_kernel<8, false, true, true>);
            else
                full ? launch(sgm_paths_wide_kernel<8, true, false, true>)
                     : launch(sgm_paths_wide_kernel<8, false, false, true>);
        } else {
            if (adapt)
                full ? launch(sgm_paths_wide_kernel<8, true, true, false>)
                     : launch(sgm_paths_wide_kernel<8, false, true, false>);
            else
                full ? launch(sgm_paths_wide_kernel<8, true, false, false>)
                     : launch(sgm_paths_wide_kernel<8, false, false, false>);
        }
    } else if (df && (num_steps & 3) == 0 && num_steps <= 128 && !wave_per_line) {
        P.dx = P.dy = 0;
        P.first = 0;
        int const pairs = sgm_grid_line_pairs(w, h);
        SgmKernelTimer timer(B.prof, stream, SMVS_SGM_K_PATHS);
        if (adapt && num_steps == 128)
            hipLaunchKernelGGL((sgm_paths2_kernel<8, true, true>), dim3(pairs), dim3(64), 0, stream, P);
        else if (adapt)
            hipLaunchKernelGGL((sgm_paths2_kernel<8, false, true>), dim3(pairs), dim3(64), 0, stream, P);
        else if (num_steps == 128)
            hipLaunchKernelGGL((sgm_paths2_kernel<8, true>), dim3(pairs), dim3(64), 0, stream, P);
        else
            hipLaunchKernelGGL((sgm_paths2_kernel<8, false>), dim3(pairs), dim3(64), 0, stream, P);
    } else if (df) {
        P.dx = P.dy = 0;
        P.first = 0;
        int const lines = sgm_grid_lines(w, h);
        SgmKernelTimer timer(B.prof, stream, SMVS_SGM_K_PATHS);
        if (adapt)
            hipLaunchKernelGGL((sgm_all_paths_kernel<16, true, true>), dim3(lines), dim3(64),
                0, stream, P);
        else
            hipLaunchKernelGGL((sgm_all_paths_kernel<16, true>), dim3(lines), dim3(64), 0,
                stream, P);
    } else if ((num_steps % 2) == 0) {
        SMVS_HIP_CHECK(hipMemsetAsync(B.sgm, 0, sizeof(uint16_t) * vol, stream));
        P.dx = P.dy = 0;
        P.first = 0;
        int const lines = sgm_grid_lines(w, h);
        SgmKernelTimer timer(B.prof, stream, SMVS_SGM_K_PATHS);
        if (adapt)
            hipLaunchKernelGGL((sgm_all_paths_kernel<16, false, true>), dim3(lines), dim3(64),
                0, stream, P);
        else
            hipLaunchKernelGGL((sgm_all_paths_kernel<16, false>), dim3(lines), dim3(64), 0,
                stream, P);
    } else {
        SgmKernelTimer timer(B.prof, stream, SMVS_SGM_K_PATHS);
        // odd plane counts: one launch per direction, scalar accesses
        for (int k = 0; k < 8; ++k) {
            P.dx = SGM_DIRS[k][0];
            P.dy = SGM_DIRS[k][1];
            P.first = k == 0 ? 1 : 0;
            int const lines = sgm_dir_lines(k, w, h);
            if (adapt)
                hipLaunchKernelGGL(sgm_path_kernel<true>, dim3(lines), dim3(64), 0, stream,
                    P);
            else
                hipLaunchKernelGGL(sgm_path_kernel<false>, dim3(lines), dim3(64), 0, stream,
                    P);
        }
    }
    SMVS_HIP_CHECK(hipGetLastError());
    {
        SgmKernelTimer timer(B.prof, stream, SMVS_SGM_K_WTA);
        if (df && num_steps > 128)
            hipLaunchKernelGGL(sgm_sum_wta_wide_kernel,
                dim3((unsigned)((npix * 64 + 255) / 256)), dim3(256), 0, stream,
                B.cost, B.delta, vol, d_main, d_depths, npix, num_steps, d_depth,
                B.argmin, B.want_sgm ? B.sgm : nullptr);
        else if (df)
            hipLaunchKernelGGL(sgm_sum_wta_kernel,
                dim3((unsigned)((npix * 32 + 255) / 256)), dim3(256), 0, stream,
                B.cost, B.delta, vol, d_main, d_depths, npix, num_steps, d_depth,
                B.argmin, B.want_sgm ? B.sgm : nullptr);
        else
            hipLaunchKernelGGL(wta_rows_kernel,
                dim3((unsigned)((npix * 16 + 255) / 256)), dim3(256), 0, stream,
                B.sgm, d_main, d_depths, npix, num_steps, d_depth,
                B.argmin);
    }
    SMVS_HIP_CHECK(hipGetLastError());
    return SMVS_OK;
}

} // namespace smvs_hip

using namespace smvs_hip;

static int
sgm_run_impl(int device, const uint8_t *main_img, int w, int h,
    const uint8_t *neighbor_img, int nw, int nh, const float *M,
    const float *t, float min_depth, float max_depth, int num_steps,
    uint16_t penalty1, uint16_t penalty2, int p2_mode, float *depth, int32_t *argmin,
    uint16_t *cost, uint16_t *sgm)
{
    SMVS_REQUIRE(main_img && neighbor_img && M && t, "null argument");
    SMVS_REQUIRE(w > 10 && h > 8 && nw > 1 && nh > 1, "image too small");
    int rc = check_sgm_options(num_steps, min_depth, max_depth, penalty1,
        penalty2, p2_mode);
    if (rc != SMVS_OK)
        return rc;
    WorkspaceLease lease(device);
    if (lease.w == nullptr)
        return SMVS_ERR_HIP;
    Workspace &ws = *lease.w;
    size_t const npix = (size_t)w * h, nnpix = (size_t)nw * nh;
    size_t const vol = npix * num_steps;
    SgmProfile prof;
    SgmWorkspace B(&ws);
    B.prof = &prof;
    B.want_sgm = sgm != nullptr;
    uint8_t *d_main = nullptr, *d_nbr = nullptr;
    float *d_depth = nullptr;
    if ((rc = ws.ensure(WS_MAIN, npix, &d_main)) || (rc = ws.ensure(WS_NBR0, nnpix, &d_nbr))
        || (rc = ws.ensure(WS_FWD0, npix, &d_depth))
        || (rc = ws.upload(d_main, main_img, npix))
        || (rc = ws.upload(d_nbr, neighbor_img, nnpix)))
        return rc;
    if ((rc = sgm_run_device(B, d_main, w, h, d_nbr, nw, nh, M, t, min_depth,
            max_depth, num_steps, penalty1, penalty2, p2_mode, d_depth)) != SMVS_OK)
        return rc;
    if (depth != nullptr
        && (rc = ws.download(depth, d_depth, sizeof(float) * npix)) != SMVS_OK)
        return rc;
    if (argmin != nullptr
        && (rc = ws.download(argmin, B.argmin, sizeof(int32_t) * npix)) != SMVS_OK)
        return rc;
    if (sgm != nullptr
        && (rc = ws.download(sgm, B.sgm, sizeof(uint16_t) * vol)) != SMVS_OK)
        return rc;
    if (cost != nullptr) {
        uint16_t *d_cost16 = nullptr;
        if ((rc = ws.ensure(WS_COST16, vol, &d_cost16)))
            return rc;
        hipLaunchKernelGGL(widen_u8_kernel, dim3((unsigned)((vol + 255) / 256)),
            dim3(256), 0, ws.stream, B.cost, d_cost16, vol);
        SMVS_HIP_CHECK(hipGetLastError());
        if ((rc = ws.download(cost, d_cost16, sizeof(uint16_t) * vol)) != SMVS_OK)
            return rc;
    }
    SMVS_HIP_CHECK(hipStreamSynchronize(ws.stream));
    return SMVS_OK;
}

extern "C" int
smvs_sgm_run(int device, const uint8_t *main_img, int w, int h,
    const uint8_t *neighbor_img, int nw, int nh, const float *M,
    const float *t, float min_depth, float max_depth, int num_steps,
    uint16_t penalty1, uint16_t penalty2, float *depth, int32_t *argmin,
    uint16_t *cost, uint16_t *sgm)
{
    return sgm_run_impl(device, main_img, w, h, neighbor_img, nw, nh, M, t, min_depth,
        max_depth, num_steps, penalty1, penalty2, SMVS_SGM_P2_CONSTANT, depth, argmin,
        cost, sgm);
}

// sgm_stereo.cc:310-346 with p2_mode = SMVS_SGM_P2_ADAPTIVE
extern "C" int
smvs_sgm_run_mode(int device, const uint8_t *main_img, int w, int h,
    const uint8_t *neighbor_img, int nw, int nh, const float *M,
    const float *t, float min_depth, float max_depth, int num_steps,
    uint16_t penalty1, uint16_t penalty2, int p2_mode, float *depth, int32_t *argmin,
    uint16_t *cost, uint16_t *sgm)
{
    return sgm_run_impl(device, main_img, w, h, neighbor_img, nw, nh, M, t, min_depth,
        max_depth, num_steps, penalty1, penalty2, p2_mode, depth, argmin, cost, sgm);
}

extern "C" int
smvs_sgm_profile(int enable, double *ms, long long *launches)
{
    std::lock_guard<std::mutex> guard(g_sgm_prof_mutex);
    for (int i = 0; i < SMVS_SGM_K_COUNT; ++i) {
        if (ms != nullptr)
            ms[i] = g_sgm_prof_ms[i];
        if (launches != nullptr)
            launches[i] = g_sgm_prof_launches[i];
    }
    if (enable >= 0) {
        // (switching it on or off starts a new measurement)
        g_sgm_prof_on = enable != 0;
        for (int i = 0; i < SMVS_SGM_K_COUNT; ++i) {
            g_sgm_prof_ms[i] = 0.0;
            g_sgm_prof_launches[i] = 0;
        }
    }
    return SMVS_OK;
}
