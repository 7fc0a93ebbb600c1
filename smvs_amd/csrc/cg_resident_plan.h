// How the resident PCG (cg_resident.hip) tiles a node grid and which of its
// two solvers runs there.  Host arithmetic only: no HIP, no smvs_ctx.
#pragma once

#include "../../include/smvs_hip.h"

#include <cstddef>

namespace smvs_hip {

constexpr int RES_THREADS = 512;
constexpr int RES_MAX_BLOCKS = 256;

// bytes of LDS a tile of tw x th nodes takes (defined beside the LDS layout,
// cg_resident.hip)
size_t resident_lds_bytes(int tw, int th, bool one);

// Tile shape: tw * th <= 512 nodes, at most max_tiles tiles, fits the LDS of
// the solver variant, smallest rim.
inline bool
choose_tiling(int stride, int rows, int max_tiles, bool one, int *tw_out, int *th_out)
{
    long best = -1;
    for (int tw = 4; tw <= 128 && tw <= RES_THREADS; ++tw) {
        int const th = RES_THREADS / tw;
        if (th < 2)
            continue;
        for (int t2 = th; t2 >= 2 && t2 >= th - 8; --t2) {
            long const tiles = (long)((stride + tw - 1) / tw)
                * ((rows + t2 - 1) / t2);
            if (tiles > max_tiles)
                continue;
            // (long thin tiles have a long rim: the one-exchange solver keeps
            // r, P and q of the halo in LDS)
            if (resident_lds_bytes(tw, t2, one) > (size_t)160 * 1024)
                continue;
            // prefer few idle threads, then a short rim
            long const waste = tiles * (long)(tw * t2) - (long)stride * rows;
            long const score = waste * 4 + tiles * (tw + t2);
            if (best < 0 || score < best) {
                best = score;
                *tw_out = tw;
                *th_out = t2;
            }
        }
    }
    return best >= 0;
}

// Which of the two resident solvers a context runs (smvs_ctx_set_solver), and
// on which tiles.  The one-exchange recurrence exists to save a grid-wide
// exchange per iteration; on a grid of ONE tile nothing is exchanged, so AUTO
// runs the reference's operation order there (conjugate_gradient.h:121-198:
// d.Ad, then r.r, z.r, x.(b + r) of the updated vectors summed directly) --
// the tiny ill-conditioned systems of the fuzz sweep live on such grids.
// SMVS_REF_ORDER_TILES=n widens that to grids of <= n tiles (measurements).
struct ResidentPlan {
    int tw, th;
    bool one;
    int blocks;     // workgroups of the launch = tiles, row-major
};

inline bool
compute_resident_plan(int stride, int rows, int max_tiles, int solver_mode,
    int ref_order_tiles, ResidentPlan *plan)
{
    int tw = 0, th = 0;
    bool one = false;
    bool const have_ref = choose_tiling(stride, rows, max_tiles, false, &tw, &th);
    bool const ref = have_ref && (solver_mode == SMVS_SOLVER_RESIDENT_REF
        || (long)((stride + tw - 1) / tw) * ((rows + th - 1) / th) <= ref_order_tiles);
    if (!ref) {
        if (!have_ref && solver_mode == SMVS_SOLVER_RESIDENT_REF)
            return false;
        if (!choose_tiling(stride, rows, max_tiles, true, &tw, &th))
            return false;
        one = true;
    }
    plan->tw = tw;
    plan->th = th;
    plan->one = one;
    plan->blocks = ((stride + tw - 1) / tw) * ((rows + th - 1) / th);
    return true;
}

} // namespace smvs_hip
