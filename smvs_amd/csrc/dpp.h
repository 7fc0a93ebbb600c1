// Cross-lane helpers on DPP (data-parallel primitives: a VALU operand taken
// from another lane, VALU latency instead of the LDS crossbar of ds_bpermute).
// wave64, rows of 16 lanes.  Used by the SGM aggregation and WTA kernels.
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

} // namespace smvs_hip
