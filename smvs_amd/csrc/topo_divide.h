// The divide-sharing arithmetic of the visibility and patch-MSE kernels
// (topo_visibility.hip, topo_mse.hip).
#pragma once

#include "topo_internal.h"

namespace smvs_hip {

// Several quotients over one denominator.  a / d as the compiler expands it is
// v_div_scale (twice), v_rcp_f64, two Newton steps on the reciprocal, the
// quotient a * r, ONE residual correction (v_div_fmas) and v_div_fixup: thirteen
// instructions, five of which depend only on d.  For a denominator well inside
// the normal range the scaling steps are the identity, so the same quotient --
// bit for bit, it is the same sequence of roundings -- comes from the shared
// refined reciprocal in three instructions plus the fix-up (zero, infinite and
// NaN numerators).  Any other denominator (zero, NaN, 1e-70 ...) is `plain ==
// false`: the caller divides.  The guarantee is conditional on the NUMERATOR
// as well: v_div_scale also rescales for numerators whose exponent is extreme
// (|a| beyond ~1e230 or denormal, quotients near overflow / underflow), and
// only the denominator is tested here.  The numerators of this file are
// projective coordinates and their pixel derivatives -- products of image
// coordinates (< 1e5), camera entries and depths, |a| < 1e20 and either exactly
// zero or > 1e-60 for any scene the surface tests accept -- so the condition
// holds; SMVS_TOPO_DIVIDE=exact runs the divisions themselves and the GPU
// suite demands identical masks.  The warp of a pixel divides ten times by d and
// d * d (Correspondence, topo_math.h): the visibility kernel issues a vector
// instruction every cycle it can, and a seventh of them were these.
struct SharedDivisor {
    double d, inv;
    bool plain;
    __device__ __forceinline__ explicit SharedDivisor(double d_, bool allow = true) : d(d_)
    {
        double const m = fabs(d_);
        plain = allow && m > 1e-70 && m < 1e70;   // (false for NaN)
        double r = __builtin_amdgcn_rcp(d_);
        r = __builtin_fma(__builtin_fma(-d_, r, 1.0), r, r);
        inv = __builtin_fma(__builtin_fma(-d_, r, 1.0), r, r);
    }
    // a / d, `plain` denominators only (no branch: straight-line callers)
    __device__ __forceinline__ double under(double a) const
    {
        double const q = a * inv;
        double const rem = __builtin_fma(-q, d, a);
        return __builtin_amdgcn_div_fixup(__builtin_fma(rem, inv, q), d, a);
    }
    // a / d for any denominator
    __device__ __forceinline__ double quotient(double a) const
    {
        return plain ? under(a) : a / d;
    }
};

// Warp::x, Warp::y and Warp::jacobian (topo_math.h; lib/correspondence.cc:20-51,
// 88-100): SHARED = the reciprocals of d and d * d computed once (only when
// plain()), otherwise the divisions of topo_math.h.  The same operations in
// the same order, every quotient the one the division gives.
template <bool SHARED>
struct WarpQuotients {
    SharedDivisor by_d, by_d2;
    __device__ __forceinline__ explicit WarpQuotients(Warp const &wp, bool allow = true)
        : by_d(wp.d, allow), by_d2(wp.d * wp.d, allow) {}
    __device__ __forceinline__ bool plain(void) const { return by_d.plain && by_d2.plain; }
    __device__ __forceinline__ double x(Warp const &wp) const
    {
        return SHARED ? by_d.under(wp.a) : wp.x();
    }
    __device__ __forceinline__ double y(Warp const &wp) const
    {
        return SHARED ? by_d.under(wp.b) : wp.y();
    }
    __device__ __forceinline__ void
    jacobian(Warp const &wp, const double *M, double w, double wx, double wy,
        double *jac) const
    {
#pragma clang fp contract(off)
        if (!SHARED) {
            wp.jacobian(M, w, wx, wy, jac);
            return;
        }
        jac[0] = by_d.under(wx * wp.p + w * M[0]) - by_d2.under(wp.a * (wx * wp.r + w * M[6]));
        jac[2] = by_d.under(wy * wp.p + w * M[1]) - by_d2.under(wp.a * (wy * wp.r + w * M[7]));
        jac[1] = by_d.under(wx * wp.q + w * M[3]) - by_d2.under(wp.b * (wx * wp.r + w * M[6]));
        jac[3] = by_d.under(wy * wp.q + w * M[4]) - by_d2.under(wp.b * (wy * wp.r + w * M[7]));
    }
};

// linear_at (topo_math.h) on both channels of a gradient plane: the taps once,
// four 8-byte loads, per channel linear_at's arithmetic term for term.
__device__ __forceinline__ void
linear_at_pair(const float2 *data, int w, int h, float x, float y, float *c0, float *c1)
{
#pragma clang fp contract(off)
    x = x < 0.0f ? 0.0f : (x > (float)(w - 1) ? (float)(w - 1) : x);
    y = y < 0.0f ? 0.0f : (y > (float)(h - 1) ? (float)(h - 1) : y);
    int const fx = (int)x, fy = (int)y;
    int const fx1 = fx + 1 < w - 1 ? fx + 1 : w - 1;
    int const fy1 = fy + 1 < h - 1 ? fy + 1 : h - 1;
    float const w1 = x - (float)fx, w0 = 1.0f - w1;
    float const w3 = y - (float)fy, w2 = 1.0f - w3;
    float2 const v00 = data[(long)fy * w + fx];
    float2 const v10 = data[(long)fy * w + fx1];
    float2 const v01 = data[(long)fy1 * w + fx];
    float2 const v11 = data[(long)fy1 * w + fx1];
    *c0 = v00.x * (w0 * w2) + v10.x * (w1 * w2) + v01.x * (w0 * w3) + v11.x * (w1 * w3);
    *c1 = v00.y * (w0 * w2) + v10.y * (w1 * w2) + v01.y * (w0 * w3) + v11.y * (w1 * w3);
}

} // namespace smvs_hip
