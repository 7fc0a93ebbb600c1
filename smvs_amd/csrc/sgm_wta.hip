// The winner-takes-all step of a run on gfx950: depth_from_sgm_volume of the
// reference (lib/sgm_stereo.cc:274-306) behind the path aggregation of
// sgm_paths.hip, as sgm_launch_wta for sgm_run_tail (sgm.hip).
//
// Three forms, by where S = sum of the eight path costs is (SgmPathPlan::wta):
// the rows form reads S from memory with 16 lanes per pixel; the two sum forms
// build S = 8 C + the eight path bytes of the DELTA form in registers, four
// planes per lane, with 32 lanes per pixel up to 128 planes and 64 above.  Each
// form with the plane's depth or the sub-plane winner, and without or with the
// uniqueness test: twelve kernels around two bodies and one store.
#include "dpp.h"
#include "sgm_internal.h"

namespace smvs_hip {

// The sub-plane winner (SMVS_SGM_WINNER_SUBPLANE; extends sgm_stereo.cc:300-303,
// not in the reference): the parabola through the winner's S = b and its two
// neighbours a, c moves the inverse depth towards the neighbouring plane on
// the lower side, by at most half a plane.  inv[k] is the inverse depth of
// plane k as sgm_stereo.cc:197-203 accumulates it (depths[k] == 1 / inv[k]), so
// an offset of 0 gives depths[i] to the bit.  The caller has excluded i < 2.
// float in the written order, contraction off, IEEE division.
__device__ __forceinline__ float
subplane_depth(int i, int a, int b, int c, const float *__restrict__ inv, int D)
{
#pragma clang fp contract(off)
    int const den = a - 2 * b + c;   // >= 0: b is the minimum
    float off = 0.0f;
    if (i != D - 1 && den != 0)
        off = (float)(a - c) / (float)(2 * den);   // in [-0.5, 0.5]
    int const n = off > 0.0f ? i + 1 : i - 1;
    float const base = inv[i];
    float const step = fabsf(off) * (inv[n] - base);
    return 1.0f / (base + step);
}

// Whether no plane of 0 .. D - 1 is more than `window` away from i.
__device__ __forceinline__ bool
no_competitor(int i, int window, int D)
{
    return i - window <= 0 && i + window >= D - 1;
}

// The end of every WTA kernel (sgm_stereo.cc:300-303): i is the winning plane,
// b its S; no depth for the two nearest planes and for dark pixels.  table: the
// depths, or with SUBPLANE the inverse depths, and a, c are S of the planes
// i - 1, i + 1 (only looked at for a valid winner, c not at all in the last
// plane).  UNIQUE, the uniqueness test of include/smvs_hip.h (not in the
// reference): r is the smallest S among the planes more than `window` away from
// i (any value without one), and no depth where
// r * (100 - uniqueness) < S[i] * 100.
template <bool SUBPLANE, bool UNIQUE>
__device__ __forceinline__ void
wta_store(int i, int a, int b, int c, uint32_t r, int window, int uniqueness, size_t p,
    const uint8_t *__restrict__ main_img, const float *__restrict__ table, int D,
    float *__restrict__ depth, int32_t *__restrict__ argmin, uint16_t *__restrict__ runner_up)
{
    bool none = true;
    if constexpr (UNIQUE) {
        none = no_competitor(i, window, D);
        if (runner_up != nullptr)
            runner_up[p] = (uint16_t)(none ? 65535u : r);
    }
    if (argmin != nullptr)
        argmin[p] = i;
    if (depth != nullptr) {
        // (r <= 65535 and b <= 65535: 32 bits)
        bool const rejected = !none && r * (uint32_t)(100 - uniqueness) < (uint32_t)b * 100u;
        float v = 0.0f;
        if (!(i < 2 || main_img[p] < 25 || rejected)) {
            if constexpr (SUBPLANE)
                v = subplane_depth(i, a, b, c, table, D);
            else
                v = table[i];
        }
        depth[p] = v;
    }
}

// Unsigned minimum over the LANES lanes of a pixel (16: a row, 32: two rows, 64:
// the wavefront), every lane of the wave taking part.  The last lane of the
// pixel ends with it; with ALL, and with 64 lanes anyway, every lane does.
template <int LANES, bool ALL>
__device__ __forceinline__ uint32_t
pixel_min_u32(uint32_t v)
{
    static_assert(LANES == 16 || LANES == 32 || LANES == 64, "rows of 16 lanes");
    if constexpr (LANES == 64) {
        // row_prefix_min_u32, then row_bcast:15 / row_bcast:31, read from lane 63
        return wave_min_u32(v);
    } else {
        v = row_prefix_min_u32(v);
        if constexpr (LANES == 32) {
            // lanes 15 and 31 of the pixel hold the row minima
            uint32_t const other = (uint32_t)__shfl_xor((int)v, 16);
            v = min(v, other);
        }
        // lane 15 of every row of the pixel holds its minimum: to the row
        if constexpr (ALL)
            v = dpp_u32<dpp_row_newbcast(15)>(v, v);
        return v;
    }
}

// The rows form (sgm_stereo.cc:274-306): S is in memory, 16 lanes per pixel,
// lane sub reads planes sub, sub + 16, ...; the first minimum wins through the
// (value, plane) key, whose low byte is the plane.  Lane 15 stores, and with
// SUBPLANE reads the winner's two neighbours from S.  UNIQUE: the winner goes to
// the 16 lanes, each takes the minimum of its planes outside the window (a
// second read of S, from the cache), a second minimum brings r to lane 15.
template <bool SUBPLANE, bool UNIQUE>
__device__ __forceinline__ void
wta_rows(const uint16_t *__restrict__ sgm, const uint8_t *__restrict__ main_img,
    const float *__restrict__ table, size_t npix, int D, int window, int uniqueness,
    float *__restrict__ depth, int32_t *__restrict__ argmin, uint16_t *__restrict__ runner_up)
{
    size_t const p = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    int const sub = threadIdx.x & 15;
    uint32_t key = 0xFFFFFFFFu;
    if (p < npix)
        for (int d = sub; d < D; d += 16)
            key = min(key, (uint32_t)sgm[p * D + d] * 256u + (uint32_t)d);
    key = pixel_min_u32<16, UNIQUE>(key);
    int const i = (int)(key & 0xFFu);
    uint32_t r = 0xFFFFFFFFu;
    if constexpr (UNIQUE) {
        if (p < npix)
            for (int d = sub; d < D; d += 16)
                if (d < i - window || d > i + window)
                    r = min(r, (uint32_t)sgm[p * D + d]);
        r = pixel_min_u32<16, false>(r);
    }
    if (sub == 15 && p < npix) {
        const uint16_t *s = sgm + p * D;
        int const a = SUBPLANE && i >= 1 ? (int)s[i - 1] : 0;
        int const c = SUBPLANE && i + 1 < D ? (int)s[i + 1] : 0;
        wta_store<SUBPLANE, UNIQUE>(i, a, (int)(key >> 8), c, r, window, uniqueness, p, main_img,
            table, D, depth, argmin, runner_up);
    }
}

// The sum forms: S = 8 C + the eight path bytes of the DELTA form and the
// winner-takes-all of wta_rows on it, LANES = 32 or 64 lanes per pixel with
// four planes each (one u32 per volume and lane).  S itself is only written
// when the caller wants the volume (smvs_sgm_run's `sgm` output).  The plane
// index uses the key's whole low byte at 256 planes; S < 2^16 keeps
// value * 256 + plane inside 32 bits.
// Without SUBPLANE and UNIQUE the last lane of the pixel stores.  With either,
// the winner's key goes to every lane of the pixel and the lane that holds the
// winning plane stores: S of the winner's neighbours is in its registers, or
// for plane 4 sub - 1 / 4 sub + 4 in the previous / next lane of the wave
// (wave_shr:1 / wave_shl:1: every 16th plane crosses a row of 16 lanes);
// UNIQUE: every lane takes the minimum of its own four sums outside the window,
// and a second cross-lane minimum gives r to every lane.
template <int LANES, bool SUBPLANE, bool UNIQUE>
__device__ __forceinline__ void
sum_wta(const uint8_t *__restrict__ cost, const uint8_t *__restrict__ delta, size_t vol,
    const uint8_t *__restrict__ main_img, const float *__restrict__ table, size_t npix, int D,
    int window, int uniqueness, float *__restrict__ depth, int32_t *__restrict__ argmin,
    uint16_t *__restrict__ runner_up, uint16_t *__restrict__ sgm_out)
{
    static_assert(LANES == 32 || LANES == 64, "half a wavefront or a whole one per pixel");
    constexpr bool ALL = SUBPLANE || UNIQUE;
    size_t const p = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / LANES;
    int const sub = threadIdx.x & (LANES - 1);
    int const d0 = 4 * sub;
    bool const mine = p < npix && d0 < D;
    uint32_t key = 0xFFFFFFFFu;
    uint32_t sv[4] = { 0u, 0u, 0u, 0u };
    if (mine) {
        size_t const o = p * (size_t)D + d0;   // D % 4 == 0: aligned u32
        uint32_t const c = *reinterpret_cast<const uint32_t *>(cost + o);
        uint32_t e[8];
#pragma unroll
        for (int k = 0; k < 8; ++k)
            e[k] = *reinterpret_cast<const uint32_t *>(delta + (size_t)k * vol + o);
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
    // (every lane of the wave takes part in the moves from here on)
    uint32_t left = 0u, right = 0u;
    if constexpr (SUBPLANE) {
        left = lane_prev(sv[3], 0u);    // S of plane d0 - 1
        right = lane_next(sv[0], 0u);   // S of plane d0 + 4
    }
    key = pixel_min_u32<LANES, ALL>(key);
    int const i = (int)(key & 0xFFu);
    uint32_t r = 0xFFFFFFFFu;
    if constexpr (UNIQUE) {
        if (mine) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                int const d = d0 + j;
                if (d < i - window || d > i + window)
                    r = min(r, sv[j]);
            }
        }
        r = pixel_min_u32<LANES, true>(r);
    }
    // (a pixel past the end has the key of all ones: plane 255, no lane of 32)
    if ((ALL ? (i >> 2) : LANES - 1) == sub && p < npix) {
        int const j = i & 3;
        uint32_t a = 0u, c = 0u;
        if constexpr (SUBPLANE) {
            // (selects, not an indexed register array)
            a = j == 0 ? left : (j == 1 ? sv[0] : (j == 2 ? sv[1] : sv[2]));
            c = j == 0 ? sv[1] : (j == 1 ? sv[2] : (j == 2 ? sv[3] : right));
        }
        wta_store<SUBPLANE, UNIQUE>(i, (int)a, (int)(key >> 8), (int)c, r, window, uniqueness, p,
            main_img, table, D, depth, argmin, runner_up);
    }
}

// ----------------------------------------------------------- the kernels
// (names, signatures and argument layouts as the launcher and the per-kernel
// records of profiles/ know them)

__global__ void __launch_bounds__(256)
wta_rows_kernel(const uint16_t *__restrict__ sgm,
    const uint8_t *__restrict__ main_img, const float *__restrict__ depths,
    size_t npix, int D, float *__restrict__ depth, int32_t *__restrict__ argmin)
{
    wta_rows<false, false>(sgm, main_img, depths, npix, D, 0, 0, depth, argmin, nullptr);
}

__global__ void __launch_bounds__(256)
wta_rows_subplane_kernel(const uint16_t *__restrict__ sgm,
    const uint8_t *__restrict__ main_img, const float *__restrict__ inv,
    size_t npix, int D, float *__restrict__ depth, int32_t *__restrict__ argmin)
{
    wta_rows<true, false>(sgm, main_img, inv, npix, D, 0, 0, depth, argmin, nullptr);
}

template <bool SUBPLANE>
__global__ void __launch_bounds__(256)
wta_rows_unique_kernel(const uint16_t *__restrict__ sgm,
    const uint8_t *__restrict__ main_img, const float *__restrict__ table,
    size_t npix, int D, int window, int uniqueness, float *__restrict__ depth,
    int32_t *__restrict__ argmin, uint16_t *__restrict__ runner_up)
{
    wta_rows<SUBPLANE, true>(sgm, main_img, table, npix, D, window, uniqueness, depth, argmin,
        runner_up);
}

__global__ void __launch_bounds__(256)
sgm_sum_wta_kernel(const uint8_t *__restrict__ cost, const uint8_t *__restrict__ delta,
    size_t vol, const uint8_t *__restrict__ main_img, const float *__restrict__ depths,
    size_t npix, int D, float *__restrict__ depth, int32_t *__restrict__ argmin,
    uint16_t *__restrict__ sgm_out)
{
    sum_wta<32, false, false>(cost, delta, vol, main_img, depths, npix, D, 0, 0, depth, argmin,
        nullptr, sgm_out);
}

__global__ void __launch_bounds__(256)
sgm_sum_wta_wide_kernel(const uint8_t *__restrict__ cost, const uint8_t *__restrict__ delta,
    size_t vol, const uint8_t *__restrict__ main_img, const float *__restrict__ depths,
    size_t npix, int D, float *__restrict__ depth, int32_t *__restrict__ argmin,
    uint16_t *__restrict__ sgm_out)
{
    sum_wta<64, false, false>(cost, delta, vol, main_img, depths, npix, D, 0, 0, depth, argmin,
        nullptr, sgm_out);
}

__global__ void __launch_bounds__(256)
sgm_sum_wta_subplane_kernel(const uint8_t *__restrict__ cost,
    const uint8_t *__restrict__ delta, size_t vol, const uint8_t *__restrict__ main_img,
    const float *__restrict__ inv, size_t npix, int D, float *__restrict__ depth,
    int32_t *__restrict__ argmin, uint16_t *__restrict__ sgm_out)
{
    sum_wta<32, true, false>(cost, delta, vol, main_img, inv, npix, D, 0, 0, depth, argmin,
        nullptr, sgm_out);
}

__global__ void __launch_bounds__(256)
sgm_sum_wta_wide_subplane_kernel(const uint8_t *__restrict__ cost,
    const uint8_t *__restrict__ delta, size_t vol, const uint8_t *__restrict__ main_img,
    const float *__restrict__ inv, size_t npix, int D, float *__restrict__ depth,
    int32_t *__restrict__ argmin, uint16_t *__restrict__ sgm_out)
{
    sum_wta<64, true, false>(cost, delta, vol, main_img, inv, npix, D, 0, 0, depth, argmin,
        nullptr, sgm_out);
}

template <int LANES, bool SUBPLANE>
__global__ void __launch_bounds__(256)
sgm_sum_wta_unique_kernel(const uint8_t *__restrict__ cost, const uint8_t *__restrict__ delta,
    size_t vol, const uint8_t *__restrict__ main_img, const float *__restrict__ table,
    size_t npix, int D, int window, int uniqueness, float *__restrict__ depth,
    int32_t *__restrict__ argmin, uint16_t *__restrict__ runner_up,
    uint16_t *__restrict__ sgm_out)
{
    sum_wta<LANES, SUBPLANE, true>(cost, delta, vol, main_img, table, npix, D, window, uniqueness,
        depth, argmin, runner_up, sgm_out);
}

// (declared in sgm_internal.h)
int
sgm_launch_wta(SgmWorkspace &B, SgmRun const &R, const uint8_t *d_main, size_t npix,
    int num_steps, float *d_depth)
{
    hipStream_t const stream = B.ws->stream;
    size_t const vol = npix * num_steps;
    bool const subplane = R.subplane;
    int const wta = R.plan.wta;
    int const lanes = wta == SGM_WTA_SUM_WIDE ? 64 : (wta == SGM_WTA_SUM ? 32 : 16);
    dim3 const grid((unsigned)((npix * lanes + 255) / 256));
    // (the sub-plane forms take the inverse depths where the others take the
    // depths)
    const float *const table = subplane ? R.d_inv : R.d_depths;
    uint16_t *const s_out = B.want_sgm ? B.sgm : nullptr;
    int const window = B.uniqueness_window, uniq = B.uniqueness;
    {
        SgmKernelTimer timer(B.prof, stream, SMVS_SGM_K_WTA);
        auto const launch = [&](auto kernel, auto... args) {
            hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, args...);
        };
        if (lanes == 16 && uniq != 0)
            launch(subplane ? wta_rows_unique_kernel<true> : wta_rows_unique_kernel<false>,
                B.sgm, d_main, table, npix, num_steps, window, uniq, d_depth, B.argmin,
                B.runner_up);
        else if (lanes == 16)
            launch(subplane ? wta_rows_subplane_kernel : wta_rows_kernel,
                B.sgm, d_main, table, npix, num_steps, d_depth, B.argmin);
        else if (uniq != 0)
            launch(lanes == 64 ? (subplane ? sgm_sum_wta_unique_kernel<64, true>
                                           : sgm_sum_wta_unique_kernel<64, false>)
                               : (subplane ? sgm_sum_wta_unique_kernel<32, true>
                                           : sgm_sum_wta_unique_kernel<32, false>),
                B.cost, B.delta, vol, d_main, table, npix, num_steps, window, uniq, d_depth,
                B.argmin, B.runner_up, s_out);
        else
            launch(lanes == 64 ? (subplane ? sgm_sum_wta_wide_subplane_kernel
                                           : sgm_sum_wta_wide_kernel)
                               : (subplane ? sgm_sum_wta_subplane_kernel : sgm_sum_wta_kernel),
                B.cost, B.delta, vol, d_main, table, npix, num_steps, d_depth, B.argmin, s_out);
    }
    SMVS_HIP_CHECK(hipGetLastError());
    return SMVS_OK;
}

} // namespace smvs_hip
