// Census and plane-sweep cost volume on gfx950 in front of the 8-path SGM
// aggregation of sgm_paths.hip and the winner-takes-all of sgm_wta.hip: one
// run_sgm, as smvs_sgm_run[_mode] and as
// sgm_run_device for a view's front end (sgm_view.hip); and the counters of the
// front end's kernel timer.
//
// Replaces SGMStereo::run_sgm (reference: lib/sgm_stereo.cc:98-124):
// census_filter (:126-148), warped_neighbors_for_depth (:150-190),
// create_cost_volume (:192-244), aggregate_sgm_costs (:429-667,
// sgm_launch_paths), depth_from_sgm_volume (:274-306, sgm_launch_wta).
//
// Integer path: results are bit-exact with the reference semantics.  The
// float warp is evaluated in the reference's operation order with FMA
// contraction off.  Volumes are [y][x][d], d fastest (sgm_stereo.cc:436-437);
// the cost volume is kept as u8 (values <= 255), S as u16.
#include "dpp.h"
#include "sgm_internal.h"

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

// (declared in sgm_internal.h)
int
check_sgm_winner(const smvs_sgm_options *opts)
{
    SMVS_REQUIRE(opts != nullptr, "null options (winner, p2_mode)");
    SMVS_REQUIRE(opts->winner == SMVS_SGM_WINNER_PLANE
            || opts->winner == SMVS_SGM_WINNER_SUBPLANE, "unknown winner");
    return SMVS_OK;
}

// (declared in sgm_internal.h)
int
check_sgm_filter(const smvs_sgm_filter_options *filter, bool run_entry)
{
    SMVS_REQUIRE(filter != nullptr,
        "null filter options (uniqueness, uniqueness_window, speckle_size, speckle_ratio)");
    SMVS_REQUIRE(filter->uniqueness >= 0 && filter->uniqueness <= 99,
        "uniqueness must be in [0, 99]");
    SMVS_REQUIRE(filter->uniqueness_window >= 1 && filter->uniqueness_window <= SGM_MAX_PLANES,
        "uniqueness_window must be in [1, 256]");
    if (int const rc = check_sgm_speckle(filter->speckle_size, filter->speckle_ratio);
        rc != SMVS_OK)
        return rc;
    if (run_entry)
        SMVS_REQUIRE(filter->speckle_size <= 1,
            "the speckle filter works on a view's final map, not on a run");
    return SMVS_OK;
}

static int
check_sgm_options(int num_steps, float min_depth, float max_depth,
    unsigned penalty1, unsigned penalty2, int p2_mode = SMVS_SGM_P2_CONSTANT)
{
    int const rc = check_sgm_plane_count(num_steps);
    if (rc != SMVS_OK)
        return rc;
    SMVS_REQUIRE(min_depth > 0.f && max_depth > min_depth, "bad depth range");
    return check_sgm_penalties(penalty1, penalty2, p2_mode);
}

// (declared in sgm_internal.h)
int
sgm_run_plan(SgmWorkspace &B, int w, int h, float min_depth, float max_depth,
    SgmRunParams const &P, SgmRun *R)
{
    int const num_steps = P.num_steps;
    int rc = check_sgm_options(num_steps, min_depth, max_depth, P.penalty1, P.penalty2,
        P.p2_mode);
    if (rc != SMVS_OK)
        return rc;
    SMVS_REQUIRE(P.winner == SMVS_SGM_WINNER_PLANE || P.winner == SMVS_SGM_WINNER_SUBPLANE,
        "unknown winner");
    R->subplane = P.winner == SMVS_SGM_WINNER_SUBPLANE;
    SMVS_REQUIRE(B.runs < SgmWorkspace::MAX_RUNS, "too many runs on one workspace");
    size_t const npix = (size_t)w * h;
    // (what decides the form of the volumes: the largest penalty2 of a step)
    R->plan = sgm_path_plan_here(num_steps,
        SgmWorkspace::largest_penalty2(P.penalty1, P.penalty2, P.p2_mode));
    if ((rc = B.ensure(npix, num_steps, R->plan)) != SMVS_OK)
        return rc;
    // sgm_stereo.cc:195-203: inverse-depth planes by repeated float addition;
    // behind the depths the inverse depths themselves, which only the sub-plane
    // winner reads
    float depths[2 * SGM_MAX_PLANES];
    float *const inv = depths + SGM_MAX_PLANES;
    {
#pragma clang fp contract(off)
        float inv_depth = 1.0f / max_depth;
        float const increment = (1.0f / min_depth - inv_depth) / (num_steps - 1);
        for (int i = 0; i < num_steps; ++i) {
            depths[i] = 1.0f / inv_depth;
            inv[i] = inv_depth;
            inv_depth += increment;
        }
    }
    float *d_depths = B.depths + 2 * SGM_MAX_PLANES * B.runs;
    R->d_depths = d_depths;
    R->d_inv = d_depths + SGM_MAX_PLANES;
    B.runs += 1;
    return B.ws->upload(d_depths, depths,
        sizeof(float) * (R->subplane ? SGM_MAX_PLANES + num_steps : num_steps));
}

// (declared in sgm_internal.h)
void
sgm_launch_census(SgmWorkspace &B, const uint8_t *d_main, int w, int h)
{
    SgmKernelTimer timer(B.prof, B.ws->stream, SMVS_SGM_K_CENSUS);
    hipLaunchKernelGGL(census_main_kernel, dim3((w + 255) / 256, h), dim3(256),
        0, B.ws->stream, d_main, w, h, B.census);
}

// (declared in sgm_internal.h)
int
sgm_launch_warp_cost(SgmWorkspace &B, SgmRun const &R, int w, int h, const uint8_t *d_nbr,
    int nw, int nh, const float *M, const float *t, int num_steps, uint8_t *d_cost)
{
    hipStream_t const stream = B.ws->stream;
    WarpArgs W;
    W.neighbor = d_nbr;
    W.nw = nw;
    W.nh = nh;
    memcpy(W.M, M, sizeof(float) * 9);
    memcpy(W.t, t, sizeof(float) * 3);
    W.depths = R.d_depths;
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
                dim3(256), 0, stream, B.warped, B.census, w, h, num_steps, d_cost);
        else
            hipLaunchKernelGGL(cost_tiled_kernel,
                dim3(tiles, (num_steps + CT_D - 1) / CT_D), dim3(256), 0, stream,
                B.warped, B.census, w, h,
                num_steps, d_cost);
    }
    SMVS_HIP_CHECK(hipGetLastError());
    return SMVS_OK;
}

// (declared in sgm_internal.h)
int
sgm_run_tail(SgmWorkspace &B, SgmRun const &R, const uint8_t *d_main, int w, int h,
    SgmRunParams const &P, float *d_depth)
{
    if (int const rc = sgm_launch_paths(B, R.plan, d_main, w, h, P); rc != SMVS_OK)
        return rc;
    // (ends with hipGetLastError)
    return sgm_launch_wta(B, R, d_main, (size_t)w * h, P.num_steps, d_depth);
}

// (declared in sgm_internal.h)
int
sgm_run_device(SgmWorkspace &B, const uint8_t *d_main, int w, int h, const uint8_t *d_nbr,
    int nw, int nh, const float *M, const float *t, float min_depth, float max_depth,
    SgmRunParams const &P, float *d_depth)
{
    SgmRun R;
    int rc = sgm_run_plan(B, w, h, min_depth, max_depth, P, &R);
    if (rc != SMVS_OK)
        return rc;
    sgm_launch_census(B, d_main, w, h);
    if ((rc = sgm_launch_warp_cost(B, R, w, h, d_nbr, nw, nh, M, t, P.num_steps, B.cost))
        != SMVS_OK)
        return rc;
    return sgm_run_tail(B, R, d_main, w, h, P, d_depth);
}

// (declared in sgm_internal.h)
int
sgm_download_cost16(Workspace &ws, const uint8_t *d_cost, size_t vol, uint16_t *cost)
{
    int rc;
    uint16_t *d_cost16 = nullptr;
    if ((rc = ws.ensure(WS_COST16, vol, &d_cost16)))
        return rc;
    hipLaunchKernelGGL(widen_u8_kernel, dim3((unsigned)((vol + 255) / 256)),
        dim3(256), 0, ws.stream, d_cost, d_cost16, vol);
    SMVS_HIP_CHECK(hipGetLastError());
    return ws.download(cost, d_cost16, sizeof(uint16_t) * vol);
}

} // namespace smvs_hip

using namespace smvs_hip;

static int
sgm_run_impl(int device, const uint8_t *main_img, int w, int h,
    const uint8_t *neighbor_img, int nw, int nh, const float *M,
    const float *t, float min_depth, float max_depth, int num_steps,
    uint16_t penalty1, uint16_t penalty2, int p2_mode, int winner, float *depth,
    int32_t *argmin, uint16_t *cost, uint16_t *sgm,
    const smvs_sgm_filter_options *filter = nullptr, uint16_t *runner_up = nullptr)
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
    B.set_filter(filter);
    if (runner_up != nullptr && (rc = ws.ensure(WS_RUNNER_UP, npix, &B.runner_up)))
        return rc;
    uint8_t *d_main = nullptr, *d_nbr = nullptr;
    float *d_depth = nullptr;
    if ((rc = ws.ensure(WS_MAIN, npix, &d_main)) || (rc = ws.ensure(WS_NBR0, nnpix, &d_nbr))
        || (rc = ws.ensure(WS_FWD0, npix, &d_depth))
        || (rc = ws.upload(d_main, main_img, npix))
        || (rc = ws.upload(d_nbr, neighbor_img, nnpix)))
        return rc;
    SgmRunParams const P = { num_steps, penalty1, penalty2, p2_mode, winner };
    if ((rc = sgm_run_device(B, d_main, w, h, d_nbr, nw, nh, M, t, min_depth, max_depth, P,
            d_depth)) != SMVS_OK)
        return rc;
    if (depth != nullptr
        && (rc = ws.download(depth, d_depth, sizeof(float) * npix)) != SMVS_OK)
        return rc;
    if (argmin != nullptr
        && (rc = ws.download(argmin, B.argmin, sizeof(int32_t) * npix)) != SMVS_OK)
        return rc;
    if (runner_up != nullptr
        && (rc = ws.download(runner_up, B.runner_up, sizeof(uint16_t) * npix)) != SMVS_OK)
        return rc;
    if (sgm != nullptr
        && (rc = ws.download(sgm, B.sgm, sizeof(uint16_t) * vol)) != SMVS_OK)
        return rc;
    if (cost != nullptr && (rc = sgm_download_cost16(ws, B.cost, vol, cost)) != SMVS_OK)
        return rc;
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
        max_depth, num_steps, penalty1, penalty2, SMVS_SGM_P2_CONSTANT,
        SMVS_SGM_WINNER_PLANE, depth, argmin, cost, sgm);
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
        max_depth, num_steps, penalty1, penalty2, p2_mode, SMVS_SGM_WINNER_PLANE, depth,
        argmin, cost, sgm);
}

// sgm_stereo.cc:274-306 with opts->winner = SMVS_SGM_WINNER_SUBPLANE
extern "C" int
smvs_sgm_run_opts(int device, const uint8_t *main_img, int w, int h,
    const uint8_t *neighbor_img, int nw, int nh, const float *M,
    const float *t, float min_depth, float max_depth, int num_steps,
    uint16_t penalty1, uint16_t penalty2, const smvs_sgm_options *opts, float *depth,
    int32_t *argmin, uint16_t *cost, uint16_t *sgm)
{
    if (int const rc = check_sgm_winner(opts); rc != SMVS_OK)
        return rc;
    return sgm_run_impl(device, main_img, w, h, neighbor_img, nw, nh, M, t, min_depth,
        max_depth, num_steps, penalty1, penalty2, opts->p2_mode, opts->winner, depth,
        argmin, cost, sgm);
}

// smvs_sgm_run_opts with the uniqueness test in the WTA step
extern "C" int
smvs_sgm_run_filtered(int device, const uint8_t *main_img, int w, int h,
    const uint8_t *neighbor_img, int nw, int nh, const float *M,
    const float *t, float min_depth, float max_depth, int num_steps,
    uint16_t penalty1, uint16_t penalty2, const smvs_sgm_options *opts,
    const smvs_sgm_filter_options *filter, float *depth, int32_t *argmin, uint16_t *cost,
    uint16_t *sgm, uint16_t *runner_up)
{
    int rc;
    if ((rc = check_sgm_winner(opts)) != SMVS_OK
        || (rc = check_sgm_filter(filter, true)) != SMVS_OK)
        return rc;
    SMVS_REQUIRE(runner_up == nullptr || filter->uniqueness != 0,
        "runner_up is an output of the uniqueness test (uniqueness > 0)");
    return sgm_run_impl(device, main_img, w, h, neighbor_img, nw, nh, M, t, min_depth,
        max_depth, num_steps, penalty1, penalty2, opts->p2_mode, opts->winner, depth,
        argmin, cost, sgm, filter, runner_up);
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
