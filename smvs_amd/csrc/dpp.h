// Cross-lane helpers on DPP (data-parallel primitives: a VALU operand taken
// from another lane, VALU latency instead of the LDS crossbar of ds_bpermute).
// wave64, rows of 16 lanes.  32-bit values for the SGM aggregation and WTA
// kernels; doubles -- two 32-bit moves joined again -- for the lane-group
// reductions of the visibility kernel (topo_visibility.hip) and the PCG solvers'
// sums (cg_exchange.h, cg.hip), with gfx950's v_permlane16_swap /
// v_permlane32_swap across the rows.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace smvs_hip {

// dpp_ctrl words: which lane an operand comes from
constexpr int DPP_ROW_SHR1 = 0x111;    // row_shr:1: lane - 1 of the same row
constexpr int DPP_ROW_SHR2 = 0x112;    // row_shr:2
constexpr int DPP_ROW_SHR4 = 0x114;    // row_shr:4
constexpr int DPP_ROW_SHR8 = 0x118;    // row_shr:8
constexpr int DPP_WAVE_SHL1 = 0x130;   // wave_shl:1: lane + 1 of the wave
constexpr int DPP_WAVE_SHR1 = 0x138;   // wave_shr:1: lane - 1 of the wave
constexpr int DPP_ROW_BCAST15 = 0x142; // row_bcast:15: lane 15 of a row to the next row
constexpr int DPP_ROW_BCAST31 = 0x143; // row_bcast:31: lane 31 to rows 2 and 3
constexpr int DPP_QUAD_SWAP1 = 0xB1;   // quad_perm [1, 0, 3, 2]: lane ^ 1
constexpr int DPP_QUAD_SWAP2 = 0x4E;   // quad_perm [2, 3, 0, 1]: lane ^ 2
constexpr int DPP_ROW_MIRROR = 0x140;  // row_mirror: lane 15 - l of the same row
constexpr int DPP_ROW_HALF_MIRROR = 0x141;   // row_half_mirror: lane 7 - l of the same half row
// quad_perm [k, k, k, k]: lane k of every quad to the quad
constexpr int dpp_quad_bcast(int k) { return k * 0x55; }
// row_ror:n: lane (l + n) mod 16 of the same row, n = 1 .. 15
constexpr int dpp_row_ror(int n) { return 0x120 + n; }
// row_newbcast:n (gfx90a and later): lane n of every row to the whole row
constexpr int dpp_row_newbcast(int n) { return 0x150 + n; }
// row_mask: the rows of 16 lanes that are written
constexpr int DPP_ROWS_ALL = 0xf;
constexpr int DPP_ROWS_1_3 = 0xa;
constexpr int DPP_ROWS_2_3 = 0xc;

// v of the lane CTRL names; a lane without a source (or outside ROW_MASK) gets
// `old`, or 0 with BOUND_CTRL
template <int CTRL, int ROW_MASK = DPP_ROWS_ALL, bool BOUND_CTRL = false>
__device__ __forceinline__ uint32_t
dpp_u32(uint32_t old, uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, CTRL, ROW_MASK, 0xf,
        BOUND_CTRL);
}

// Unsigned prefix minimum inside each row of 16 lanes: lane 15 of a row ends
// with the row's minimum.
__device__ __forceinline__ uint32_t
row_prefix_min_u32(uint32_t v)
{
    uint32_t const ident = 0xFFFFFFFFu;
    v = min(v, dpp_u32<DPP_ROW_SHR1>(ident, v));
    v = min(v, dpp_u32<DPP_ROW_SHR2>(ident, v));
    v = min(v, dpp_u32<DPP_ROW_SHR4>(ident, v));
    v = min(v, dpp_u32<DPP_ROW_SHR8>(ident, v));
    return v;
}

// Wave-wide unsigned minimum: the prefix minimum of the rows, row_bcast:15 /
// row_bcast:31 to combine the rows, total in lane 63.
__device__ __forceinline__ uint32_t
wave_min_u32(uint32_t v)
{
    uint32_t const ident = 0xFFFFFFFFu;
    v = row_prefix_min_u32(v);
    v = min(v, dpp_u32<DPP_ROW_BCAST15, DPP_ROWS_1_3>(ident, v));
    v = min(v, dpp_u32<DPP_ROW_BCAST31, DPP_ROWS_2_3>(ident, v));
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// value of the previous / next lane; lanes without a source get `fill`
__device__ __forceinline__ uint32_t
lane_prev(uint32_t v, uint32_t fill)
{
    return dpp_u32<DPP_WAVE_SHR1>(fill, v);
}

__device__ __forceinline__ uint32_t
lane_next(uint32_t v, uint32_t fill)
{
    return dpp_u32<DPP_WAVE_SHL1>(fill, v);
}

// max over a DPP pattern with bound_ctrl: a lane without a source reads 0, the
// identity of an unsigned maximum -- one v_max_u32_dpp, nothing to move into
// the destination first (sgm_paths2_kernel takes its minimum as the maximum of
// the complements)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t
max_dpp0(uint32_t v)
{
    return max(v, dpp_u32<CTRL, ROW_MASK, true>(0u, v));
}

// Wave-wide unsigned maximum on max_dpp0, the same in every lane: the prefix
// maximum of the rows, row_bcast:15 / row_bcast:31 to combine the four rows,
// the total read from lane 63 (sgm_paths_wide_kernel's minimum over a line of
// 64 lanes, as the maximum of the complements)
__device__ __forceinline__ uint32_t
wave_max_dpp0(uint32_t v)
{
    v = max_dpp0<DPP_ROW_SHR1, DPP_ROWS_ALL>(v);
    v = max_dpp0<DPP_ROW_SHR2, DPP_ROWS_ALL>(v);
    v = max_dpp0<DPP_ROW_SHR4, DPP_ROWS_ALL>(v);
    v = max_dpp0<DPP_ROW_SHR8, DPP_ROWS_ALL>(v);
    v = max_dpp0<DPP_ROW_BCAST15, DPP_ROWS_1_3>(v);
    v = max_dpp0<DPP_ROW_BCAST31, DPP_ROWS_2_3>(v);
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// ---- doubles: the two words of the value moved separately ----
__device__ __forceinline__ double
join_words(unsigned lo, unsigned hi)
{
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// v of the lane CTRL names.  A lane without a source gets 0.0; BOUND_CTRL says
// how: false moves into a zeroed destination (v_mov_b32 0, then the DPP move),
// true is the bare move with bound_ctrl (__builtin_amdgcn_mov_dpp) -- the
// patterns that give every lane a source compile to the same either way.
template <int CTRL, bool BOUND_CTRL = false>
__device__ __forceinline__ double
dpp_f64(double v)
{
    unsigned long long const b = (unsigned long long)__double_as_longlong(v);
    int lo, hi;
    if constexpr (BOUND_CTRL) {
        lo = __builtin_amdgcn_mov_dpp((int)(unsigned)b, CTRL, DPP_ROWS_ALL, 0xf, true);
        hi = __builtin_amdgcn_mov_dpp((int)(unsigned)(b >> 32), CTRL, DPP_ROWS_ALL, 0xf, true);
    } else {
        lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)b, CTRL, DPP_ROWS_ALL, 0xf, false);
        hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(b >> 32), CTRL, DPP_ROWS_ALL, 0xf,
            false);
    }
    return join_words((unsigned)lo, (unsigned)hi);
}

// v_permlane32_swap (HALF = 32: lane l of the lower half of the wave and lane
// l + 32) resp. v_permlane16_swap (HALF = 16: the even and the odd rows of 16
// lanes).  Both values of every pair, the lower lane's first: a lower lane
// gets (its x, the upper lane's x), an upper lane (the lower lane's y, its y)
// -- with y = x every lane has the pair's two values, with another y the two
// halves work on two quantities at once (one step of a reduce-scatter).
template <int HALF>
__device__ __forceinline__ void
permlane_swap_f64(double x, double y, double &lower, double &upper)
{
    static_assert(HALF == 16 || HALF == 32, "rows or halves of the wave");
    typedef unsigned int u2 __attribute__((ext_vector_type(2)));
    unsigned long long const xb = (unsigned long long)__double_as_longlong(x);
    unsigned long long const yb = (unsigned long long)__double_as_longlong(y);
    u2 lo, hi;
    if constexpr (HALF == 32) {
        lo = __builtin_amdgcn_permlane32_swap((unsigned)xb, (unsigned)yb, false, false);
        hi = __builtin_amdgcn_permlane32_swap((unsigned)(xb >> 32), (unsigned)(yb >> 32),
            false, false);
    } else {
        lo = __builtin_amdgcn_permlane16_swap((unsigned)xb, (unsigned)yb, false, false);
        hi = __builtin_amdgcn_permlane16_swap((unsigned)(xb >> 32), (unsigned)(yb >> 32),
            false, false);
    }
    // .x: [x of the lower half | y of the lower half], .y: [x of the upper half |
    // y of the upper half]
    lower = join_words(lo.x, hi.x);
    upper = join_words(lo.y, hi.y);
}

} // namespace smvs_hip
