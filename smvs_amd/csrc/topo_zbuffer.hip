// The z-buffers of create_subview_surfaces (lib/depth_optimizer.cc:441-470): the
// current surface (and the SGM depth) splatted into every neighbour, then the
// minimum filter the visibility test reads (topology.hip has the overview).
#include "topo_internal.h"

#include <algorithm>

namespace smvs_hip {

// the per-centre minima of every neighbour's z-buffer start at 10000
// (depth_optimizer.cc:441-446)
__global__ void __launch_bounds__(256)
topo_clear_kernel(TopoArgs A)
{
    int const s = blockIdx.z;
    TopoView const sv = A.views[1 + s];
    size_t const cells = (size_t)(sv.w + 1) * (sv.h + 1);
    size_t const i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < cells)
        A.zraw[s][i] = 10000.0f;
    // ... and the masks the visibility kernel ORs into start at zero (the first
    // neighbour's blocks; one runtime fill kernel per call less)
    if (s == 0)
        for (size_t p = i; p < (size_t)A.num_patches; p += (size_t)gridDim.x * blockDim.x)
            A.vis_out[p] = 0u;
}

// ---- z-buffer splat (depth_optimizer.cc:441-470), one thread per pixel ----
__global__ void __launch_bounds__(256)
topo_splat_kernel(TopoArgs A)
{
    int const x = blockIdx.x * blockDim.x + threadIdx.x;
    int const y = blockIdx.y;
    if (x >= A.W || y >= A.H)
        return;
    float depths[2] = { 0.0f, 0.0f };
    // Surface::get_depth_map (surface.cc:155-168): float of the patch value
    int const gx = x - A.start_x, gy = y - A.start_y;
    if (gx >= 0 && gy >= 0 && gx < A.npx * A.ps && gy < A.npy * A.ps) {
        int const ix = gx >> A.ps_log2, iy = gy >> A.ps_log2;
        int const p = iy * A.npx + ix;
        if (A.patch_valid[p]) {
            double n16[16];
            load_patch_nodes(A, p, n16);
            int const i = gx - ix * A.ps, j = gy - iy * A.ps;
            depths[0] = (float)smvs_topo::patch_eval(n16, (i + 0.5) * A.inv_ps,
                (j + 0.5) * A.inv_ps, 0, 0);
        }
    }
    if (A.sgm_depth != nullptr)
        depths[1] = A.sgm_depth[(size_t)y * A.W + x];
    // Round 6: the two depths of a pixel (the surface's and the SGM map's) mostly
    // land in the same cell of a neighbour -- the surface starts as the SGM map --
    // and the L2 serves one atomic per clock and channel, 32 M of them per call
    // with SGM: where both centres agree ONE atomic carries the smaller depth (the
    // minimum is exact and order free, so the buffer is the same to the bit).
    bool const on[2] = { depths[0] != 0.0f, depths[1] != 0.0f };   // (NaN splats like the reference: no effect)
    if (!on[0] && !on[1])
        return;
    for (int s = 0; s < A.n_subs; ++s) {
        int const sw = A.views[1 + s].w, sh = A.views[1 + s].h;
        size_t cell[2] = { 0, 0 };
        float df[2] = { 0.0f, 0.0f };
        bool hit[2] = { false, false };
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (!on[k])
                continue;
            double const w = depths[k];
            Warp wp(A.cams->M[s], A.cams->t[s], x + 0.5, y + 0.5, w);
            double const qx = wp.x() - 0.5, qy = wp.y() - 0.5;
            double const cutoffset = 3.0;
            if (qx < cutoffset || qx >= sw - cutoffset || qy < cutoffset
                || qy >= sh - cutoffset)
                continue;
            int const cx = (int)qx, cy = (int)qy;
            df[k] = (float)wp.d;
            if (!(df[k] == df[k]))
                continue;
            // The reference writes df into the 3 x 3 cells around (cx, cy)
            // (:455-462).  min is exact and order free, so the same buffer is
            // the 3 x 3 minimum filter of the per-centre minima: one atomic per
            // (pixel, neighbour) here instead of nine, the dilate kernel does
            // the rest.
            cell[k] = (size_t)cy * (sw + 1) + cx;
            hit[k] = true;
        }
        if (hit[0] && hit[1] && cell[0] == cell[1]) {
            atomic_min_float(A.zraw[s] + cell[0], fminf(df[0], df[1]));
        } else {
            if (hit[0])
                atomic_min_float(A.zraw[s] + cell[0], df[0]);
            if (hit[1])
                atomic_min_float(A.zraw[s] + cell[1], df[1]);
        }
    }
}

// zbuf = 3 x 3 minimum filter of zraw (cells outside the buffer do not exist).
// The minimum is separable and exact: a thread takes DILATE_ROWS rows of one
// column, forms the three-column minimum of the DILATE_ROWS + 2 rows it needs
// once and combines three of them per output: 4.5 loads per cell instead of 9
// (the kernel is bound by its cached loads).
constexpr int DILATE_ROWS = 4;
__global__ void __launch_bounds__(256)
topo_dilate_kernel(TopoArgs A)
{
    int const s = blockIdx.z;
    int const zw = A.views[1 + s].w + 1, zh = A.views[1 + s].h + 1;
    int const x = blockIdx.x * blockDim.x + threadIdx.x;
    int const y0 = blockIdx.y * DILATE_ROWS;
    if (x >= zw || y0 >= zh)
        return;
    const float *raw = A.zraw[s];
    float rows[DILATE_ROWS + 2];
#pragma unroll
    for (int r = 0; r < DILATE_ROWS + 2; ++r) {
        int const yy = y0 - 1 + r;
        float m = 10000.0f;
        if (yy >= 0 && yy < zh) {
            const float *row = raw + (size_t)yy * zw;
            m = fminf(m, row[x]);
            if (x > 0)
                m = fminf(m, row[x - 1]);
            if (x + 1 < zw)
                m = fminf(m, row[x + 1]);
        }
        rows[r] = m;
    }
#pragma unroll
    for (int r = 0; r < DILATE_ROWS; ++r)
        if (y0 + r < zh)
            A.zbuf[s][(size_t)(y0 + r) * zw + x]
                = fminf(fminf(rows[r], rows[r + 1]), rows[r + 2]);
}

// The visibility test looks at the 3 x 3 z-buffer cells around a pixel's
// projection and fails when ANY of them is nearer than 0.95 of the pixel's depth
// (depth_optimizer.cc:792-830) -- i.e. when their MINIMUM is: a > b_i for some i
// <=> a > min b_i (no NaN is ever splatted).  The minimum of 3 x 3 cells of the
// 3 x 3 minimum filter is the 5 x 5 minimum filter of zraw, so this kernel leaves
// THAT in zbuf and the test is one lookup per (pixel, neighbour) instead of nine
// (round 6: 16 M x 9 four-byte loads per call at 1920 x 1080 x 8 were most of the
// vector-memory instructions of the visibility kernel's pixel pass).  Cells
// outside the buffer do not exist, as in the 3 x 3 filter; the test only looks
// at cells whose 3 x 3 neighbourhood is inside (its 3 % border).
// A workgroup loads DIL5_ROWS + 4 rows of 256 columns once (coalesced, into
// LDS), forms the five-column minima per row and the five-row minima of those:
// 252 x DIL5_ROWS cells per workgroup, 1.5 loads per cell.
constexpr int DIL5_ROWS = 8;
constexpr int DIL5_COLS = 252;
__global__ void __launch_bounds__(256)
topo_dilate5_kernel(TopoArgs A)
{
    __shared__ float tile[DIL5_ROWS + 4][256];
    int const s = blockIdx.z;
    int const zw = A.views[1 + s].w + 1, zh = A.views[1 + s].h + 1;
    int const t = (int)threadIdx.x;
    int const x0 = (int)blockIdx.x * DIL5_COLS;        // first output column; tile column j is x0 - 2 + j
    int const y0 = (int)blockIdx.y * DIL5_ROWS;
    if (x0 >= zw || y0 >= zh)
        return;
    const float *raw = A.zraw[s];
    int const gx = x0 - 2 + t;
    bool const col_ok = gx >= 0 && gx < zw;
#pragma unroll
    for (int r = 0; r < DIL5_ROWS + 4; ++r) {
        int const gy = y0 - 2 + r;
        // (a cell that does not exist takes no part in a minimum: +inf)
        tile[r][t] = col_ok && gy >= 0 && gy < zh ? raw[(size_t)gy * zw + gx] : __builtin_inff();
    }
    __syncthreads();
    if (t < 2 || t >= 2 + DIL5_COLS || gx >= zw)
        return;
    float rows[DIL5_ROWS + 4];
#pragma unroll
    for (int r = 0; r < DIL5_ROWS + 4; ++r)
        rows[r] = fminf(fminf(fminf(tile[r][t - 2], tile[r][t - 1]), tile[r][t]),
            fminf(tile[r][t + 1], tile[r][t + 2]));
#pragma unroll
    for (int r = 0; r < DIL5_ROWS; ++r)
        if (y0 + r < zh)
            A.zbuf[s][(size_t)(y0 + r) * zw + gx] = fminf(fminf(fminf(rows[r], rows[r + 1]),
                rows[r + 2]), fminf(rows[r + 3], rows[r + 4]));
}

void
launch_zbuffers(smvs_ctx *ctx, TopoArgs const &A)
{
    {
        // every neighbour's per-centre minima start at 10000 (one launch; a
        // memset per neighbour is two runtime kernels each)
        size_t cells = 0;
        for (int s = 0; s < ctx->n_subs; ++s)
            cells = std::max(cells, (size_t)(ctx->images[1 + s].w + 1)
                * (ctx->images[1 + s].h + 1));
        hipLaunchKernelGGL(topo_clear_kernel, dim3((unsigned)((cells + 255) / 256), 1,
            (unsigned)ctx->n_subs), dim3(256), 0, ctx->stream, A);
    }
    hipLaunchKernelGGL(topo_splat_kernel, dim3((ctx->width + 255) / 256,
        ctx->height), dim3(256), 0, ctx->stream, A);
    {
        int zw = 0, zh = 0;
        for (int s = 0; s < ctx->n_subs; ++s) {
            zw = std::max(zw, ctx->images[1 + s].w + 1);
            zh = std::max(zh, ctx->images[1 + s].h + 1);
        }
        // (column blocks padded to a multiple of 8: vertically adjacent row blocks
        // then share an XCD's L2, csrc/scale.hip launch_blur_ks)
        if (A.zbuf5)
            hipLaunchKernelGGL(topo_dilate5_kernel,
                dim3((((unsigned)zw + DIL5_COLS - 1) / DIL5_COLS + 7u) & ~7u,
                    (zh + DIL5_ROWS - 1) / DIL5_ROWS, ctx->n_subs), dim3(256), 0, ctx->stream, A);
        else
            hipLaunchKernelGGL(topo_dilate_kernel, dim3((((unsigned)zw + 255u) / 256u + 7u) & ~7u,
                (zh + DILATE_ROWS - 1) / DILATE_ROWS, ctx->n_subs), dim3(256), 0, ctx->stream, A);
    }
}

} // namespace smvs_hip
