// The bicubic patch at a pixel: eval_patch (value and first derivatives,
// surface_maps.hip) and eval_patch_column + eval_patch_row (the value alone,
// reactivate.hip).  The value has the same bits from both.
#pragma once

namespace smvs_hip {

// bicubic value / first derivatives at pixel (ci, cj) of a patch from the
// 1-D Hermite table rows (global memory, [ps][12]).
__device__ __forceinline__ void
eval_patch(const double *tab, int ci, int cj, double const theta[16],
    double *w, double *wx, double *wy)
{
    const double *X = tab + (size_t)ci * 12;
    const double *Y = tab + (size_t)cj * 12;
    double v = 0.0, vx = 0.0, vy = 0.0;
#pragma unroll
    for (int ey = 0; ey < 4; ++ey) {
        double g0 = 0.0, g1 = 0.0;
#pragma unroll
        for (int ex = 0; ex < 4; ++ex) {
            int const a = ex & 1, ix = ex >> 1, b = ey & 1, iy = ey >> 1;
            double const c = theta[4 * (2 * b + a) + ix + 2 * iy];
            g0 = __builtin_fma(c, X[ex * 3 + 0], g0);
            g1 = __builtin_fma(c, X[ex * 3 + 1], g1);
        }
        v = __builtin_fma(g0, Y[ey * 3 + 0], v);
        vx = __builtin_fma(g1, Y[ey * 3 + 0], vx);
        vy = __builtin_fma(g0, Y[ey * 3 + 1], vy);
    }
    *w = v;
    *wx = vx;
    *wy = vy;
}

// The sixteen x-direction FMAs of eval_patch's value: they depend only on the
// pixel's column, so a thread that owns several rows of one column forms them
// once.  Same operations in the same order as eval_patch (explicit FMAs): the
// bits of the value are the same.
__device__ __forceinline__ void
eval_patch_column(const double *tab, int ci, double const theta[16], double g[4])
{
    const double *X = tab + (size_t)ci * 12;
#pragma unroll
    for (int ey = 0; ey < 4; ++ey) {
        double g0 = 0.0;
#pragma unroll
        for (int ex = 0; ex < 4; ++ex) {
            int const a = ex & 1, ix = ex >> 1, b = ey & 1, iy = ey >> 1;
            g0 = __builtin_fma(theta[4 * (2 * b + a) + ix + 2 * iy], X[ex * 3 + 0], g0);
        }
        g[ey] = g0;
    }
}

// ... and the four y-direction FMAs that finish the value at row cj
__device__ __forceinline__ double
eval_patch_row(const double *tab, int cj, double const g[4])
{
    const double *Y = tab + (size_t)cj * 12;
    double v = 0.0;
#pragma unroll
    for (int ey = 0; ey < 4; ++ey)
        v = __builtin_fma(g[ey], Y[ey * 3 + 0], v);
    return v;
}

} // namespace smvs_hip
