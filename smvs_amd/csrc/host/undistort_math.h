// Arithmetic shared by the host form (g++, csrc/host/colmap_io.cc) and the
// device kernel (hipcc, csrc/undistort.hip) of the undistortion resampling
// (smvs_undistort_u8, include/smvs_hip.h): where an output pixel of the pinhole
// camera looks in the source image, and the bilinear sample there.  One source
// for both sides: plain IEEE float operations in source order, one rounding
// per operation, no contraction.
#ifndef SMVS_UNDISTORT_MATH_H
#define SMVS_UNDISTORT_MATH_H

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define SMVS_UND_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#define SMVS_UND_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define SMVS_UND_HD inline
#define SMVS_UND_NO_CONTRACT
#endif

namespace smvs_undistort {

// The source camera (smvs_lens) and the output camera, with everything that
// does not depend on the pixel formed once.
struct Mapping
{
    float fx, fy, cx, cy, k1, k2;
    float p1, p2, two_p1, two_p2;   // 2.0f * p1, 2.0f * p2
    float inv;                      // (float)(1.0 / (double)out_focal)
    float half_w, half_h;           // 0.5f * (float)out_width, 0.5f * (float)out_height
    float max_x, max_y;             // (float)(width - 1), (float)(height - 1)
    int width, height;              // source image
};

SMVS_UND_HD Mapping
make_mapping(float fx, float fy, float cx, float cy, float k1, float k2, float p1,
    float p2, int width, int height, float out_focal, int out_width, int out_height)
{
    SMVS_UND_NO_CONTRACT
    Mapping m;
    m.fx = fx; m.fy = fy; m.cx = cx; m.cy = cy; m.k1 = k1; m.k2 = k2;
    m.p1 = p1; m.p2 = p2;
    m.two_p1 = 2.0f * p1;
    m.two_p2 = 2.0f * p2;
    m.inv = (float)(1.0 / (double)out_focal);
    m.half_w = 0.5f * (float)out_width;
    m.half_h = 0.5f * (float)out_height;
    m.max_x = (float)(width - 1);
    m.max_y = (float)(height - 1);
    m.width = width;
    m.height = height;
    return m;
}

// Output pixel (x, y) -> source position (*sx, *sy) in pixel-index units (the
// centre of source pixel (0, 0) is (0, 0) here; COLMAP's (0.5, 0.5) is taken
// off at the end).  true: inside, 0 <= sx <= width - 1 and 0 <= sy <= height - 1
// (a NaN compares false: outside).
SMVS_UND_HD bool
source_position(Mapping const& m, int x, int y, float* sx, float* sy)
{
    SMVS_UND_NO_CONTRACT
    float const u = (((float)x + 0.5f) - m.half_w) * m.inv;
    float const v = (((float)y + 0.5f) - m.half_h) * m.inv;
    float const uu = u * u;
    float const vv = v * v;
    float const r2 = uu + vv;
    float const uv = u * v;
    float const rad = 1.0f + r2 * (m.k1 + m.k2 * r2);
    float const du = m.two_p1 * uv + m.p2 * (r2 + 2.0f * uu);
    float const dv = m.p1 * (r2 + 2.0f * vv) + m.two_p2 * uv;
    *sx = ((m.fx * (u * rad + du)) + m.cx) - 0.5f;
    *sy = ((m.fy * (v * rad + dv)) + m.cy) - 0.5f;
    return *sx >= 0.0f && *sx <= m.max_x && *sy >= 0.0f && *sy <= m.max_y;
}

// The four taps of an inside position and their weights
struct Taps
{
    std::size_t o00, o10, o01, o11;   // byte offsets of channel 0
    float w0, w1, w2, w3;
};

SMVS_UND_HD Taps
make_taps(Mapping const& m, int channels, float sx, float sy)
{
    SMVS_UND_NO_CONTRACT
    int const x0 = (int)sx, y0 = (int)sy;
    int const x1 = x0 + 1 < m.width - 1 ? x0 + 1 : m.width - 1;
    int const y1 = y0 + 1 < m.height - 1 ? y0 + 1 : m.height - 1;
    std::size_t const rowbytes = (std::size_t)m.width * (std::size_t)channels;
    Taps t;
    t.o00 = (std::size_t)y0 * rowbytes + (std::size_t)x0 * (std::size_t)channels;
    t.o10 = (std::size_t)y0 * rowbytes + (std::size_t)x1 * (std::size_t)channels;
    t.o01 = (std::size_t)y1 * rowbytes + (std::size_t)x0 * (std::size_t)channels;
    t.o11 = (std::size_t)y1 * rowbytes + (std::size_t)x1 * (std::size_t)channels;
    t.w1 = sx - (float)x0;
    t.w0 = 1.0f - t.w1;
    t.w3 = sy - (float)y0;
    t.w2 = 1.0f - t.w3;
    return t;
}

// Image<uint8_t>::linear_at of one channel: the products left to right, the
// sum left to right, + 0.5f, truncated
SMVS_UND_HD uint8_t
sample(const uint8_t* src, Taps const& t, int ch)
{
    SMVS_UND_NO_CONTRACT
    float const v00 = (float)src[t.o00 + (std::size_t)ch];
    float const v10 = (float)src[t.o10 + (std::size_t)ch];
    float const v01 = (float)src[t.o01 + (std::size_t)ch];
    float const v11 = (float)src[t.o11 + (std::size_t)ch];
    float const s = v00 * t.w0 * t.w2 + v10 * t.w1 * t.w2 + v01 * t.w0 * t.w3
        + v11 * t.w1 * t.w3;
    return (uint8_t)(s + 0.5f);
}

} // namespace smvs_undistort

#endif
