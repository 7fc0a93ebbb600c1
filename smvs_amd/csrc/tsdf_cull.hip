// The brick cull of the brick-sparse fusion on gfx950 (DESIGN.md section 9.10;
// opt-in).  The normative definition is the comment of
// smvs_tsdf_fuse_sparse_opts in include/smvs_hip.h, restated by tests/
// tsdf_cull_ref.py: per view a min/max pyramid of D, per brick a conservative
// test against it that drops only bricks which provably hold no seed, and the
// exact seed test of tsdf_sparse.hip on the bricks that are left.
//   pyramid tile  one block per 32 x 32 pixels of a view: levels 1-5 of the
//                 tile through LDS
//   pyramid top   one block per view: levels 6 .. 1 x 1 from level 5
//   cull          one lane per brick, the views in a loop: a byte per brick and
//                 the candidates per 256 bricks
//   scan          export_common.hip's exclusive_scan over those counts
//   list          rank -> brick, in brick order
//   seed (list)   tsdf_sparse_seed_kernel's body, one block per listed brick
// Arithmetic: the pyramid is float min / max (exact); the test is double, FMA
// contraction off, one operation per operation of the definition.  No atomics,
// no scratch.
#include "common.h"
#include "mesh_shared.h"
#include "tsdf_shared.h"

#include <cmath>
#include <vector>

namespace smvs_hip {

constexpr int PYR_TILE = 32;          // pixels per side of a tile: levels 1-5
constexpr int PYR_TILE_LEVELS = 5;

__device__ __forceinline__ int
pyramid_side(int n, int level)
{
    return (int)(((unsigned)n + (1u << level) - 1u) >> level);
}

// level 0: a pixel is valid where D is neither 0 nor NaN
__device__ __forceinline__ void
pyramid_pixel(float D, float &lo, float &hi)
{
    if (D > 0.0f || D < 0.0f) {
        lo = fminf(lo, D);
        hi = fmaxf(hi, D);
    }
}

__global__ void __launch_bounds__(256)
tsdf_pyramid_tile_kernel(const MeshViewDev *__restrict__ views,
    const TsdfPyramidDev *__restrict__ pyramids)
{
    // levels 1-5 of the tile: 16 x 16, 8 x 8, 4 x 4, 2 x 2, 1
    __shared__ float2 tile[256 + 64 + 16 + 4 + 1];
    MeshViewDev const &V = views[blockIdx.y];
    TsdfPyramidDev const &P = pyramids[blockIdx.y];
    int const w = V.w, h = V.h;
    unsigned const tiles_x = (unsigned)(w + PYR_TILE - 1) / PYR_TILE,
        tiles_y = (unsigned)(h + PYR_TILE - 1) / PYR_TILE;
    if (blockIdx.x >= tiles_x * tiles_y)
        return;
    int const tx = (int)(blockIdx.x % tiles_x), ty = (int)(blockIdx.x / tiles_x);
    float const inf = __builtin_huge_valf();
    float lo = inf, hi = -inf;
    {
        int const x0 = tx * PYR_TILE + 2 * (int)(threadIdx.x & 15),
            y0 = ty * PYR_TILE + 2 * (int)(threadIdx.x >> 4);
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            int const x = x0 + (d & 1), y = y0 + (d >> 1);
            if (x < w && y < h)
                pyramid_pixel(V.depth_z[(size_t)y * w + x], lo, hi);
        }
    }
    int src = 0, dst = 0;
#pragma unroll
    for (int level = 1; level <= PYR_TILE_LEVELS; ++level) {
        int const side = PYR_TILE >> level;          // texels per side of the tile
        if (level > 1) {
            lo = inf;
            hi = -inf;
            if ((int)threadIdx.x < side * side) {
                int const lx = 2 * (int)(threadIdx.x % side), ly = 2 * (int)(threadIdx.x / side);
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    float2 const t = tile[src + (ly + (d >> 1)) * 2 * side + lx + (d & 1)];
                    lo = fminf(lo, t.x);
                    hi = fmaxf(hi, t.y);
                }
            }
        }
        if ((int)threadIdx.x < side * side) {
            tile[dst + threadIdx.x] = make_float2(lo, hi);
            int const x = tx * side + (int)(threadIdx.x % side),
                y = ty * side + (int)(threadIdx.x / side);
            int const wl = pyramid_side(w, level), hl = pyramid_side(h, level);
            if (level <= P.levels && x < wl && y < hl)
                P.texels[(size_t)P.off[level] + (size_t)y * wl + x] = make_float2(lo, hi);
        }
        __syncthreads();
        src = dst;
        dst += side * side;
    }
}

// levels 6 .. P.levels of one view, each from the one below it
__global__ void __launch_bounds__(256)
tsdf_pyramid_top_kernel(const MeshViewDev *__restrict__ views,
    const TsdfPyramidDev *__restrict__ pyramids)
{
    MeshViewDev const &V = views[blockIdx.x];
    TsdfPyramidDev const &P = pyramids[blockIdx.x];
    float const inf = __builtin_huge_valf();
    for (int level = PYR_TILE_LEVELS + 1; level <= P.levels; ++level) {
        int const ws = pyramid_side(V.w, level - 1), hs = pyramid_side(V.h, level - 1);
        int const wd = pyramid_side(V.w, level), hd = pyramid_side(V.h, level);
        const float2 *from = P.texels + P.off[level - 1];
        float2 *to = P.texels + P.off[level];
        for (size_t e = threadIdx.x; e < (size_t)wd * hd; e += 256) {
            int const x = 2 * (int)(e % wd), y = 2 * (int)(e / wd);
            float lo = inf, hi = -inf;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                int const sx = x + (d & 1), sy = y + (d >> 1);
                if (sx < ws && sy < hs) {
                    float2 const t = from[(size_t)sy * ws + sx];
                    lo = fminf(lo, t.x);
                    hi = fmaxf(hi, t.y);
                }
            }
            to[e] = make_float2(lo, hi);
        }
        // the level is read by other threads of this block
        __threadfence_block();
        __syncthreads();
    }
}

// ----------------------------------------------------------------------- cull
// the pixel range of one image axis (definition: "Otherwise"); false: outside
__device__ __forceinline__ bool
cull_range(double p_lo, double p_hi, double zlo, double zhi, int n, int &first, int &last)
{
#pragma clang fp contract(off)
    double ulo = fmin(p_lo / zlo, p_lo / zhi), uhi = fmax(p_hi / zlo, p_hi / zhi);
    ulo = fmin(fmax(ulo, -4.0), (double)n + 4.0);
    uhi = fmin(fmax(uhi, -4.0), (double)n + 4.0);
    first = (int)floor(ulo) - 1;
    last = (int)floor(uhi) + 1;
    if (last < 0 || first > n - 1)
        return false;
    first = first < 0 ? 0 : first;
    last = last > n - 1 ? n - 1 : last;
    return true;
}

__device__ __forceinline__ bool
cull_finite(double x)
{
    return fabs(x) < __builtin_huge_val();
}

// may the view seed a voxel of the box [lo, hi]?
__device__ __forceinline__ bool
cull_view(MeshViewDev const &V, TsdfPyramidDev const &P, const double *lo, const double *hi,
    double T)
{
#pragma clang fp contract(off)
    double p_lo[3], p_hi[3];
    bool finite = true;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        double const t = (double)V.t[r];
        double a = 0.0, b = 0.0, mag = fabs(t);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            double const m = (double)V.KR[3 * r + k];
            double const p = m * lo[k], q = m * hi[k];
            a = a + fmin(p, q);
            b = b + fmax(p, q);
            mag = mag + fabs(m) * fmax(fabs(lo[k]), fabs(hi[k]));
        }
        double const e = 0x1p-21 * mag + 0x1p-140;
        p_lo[r] = (a - t) - e;
        p_hi[r] = (b - t) + e;
        finite = finite && cull_finite(p_lo[r]) && cull_finite(p_hi[r]);
    }
    if (!finite)
        return true;
    double const zlo = p_lo[2], zhi = p_hi[2];
    if (zhi <= 0.0)
        return false;
    int const w = V.w, h = V.h;
    int x0 = 0, x1 = w - 1, y0 = 0, y1 = h - 1;
    if (zlo > 0.0) {
        if (!cull_range(p_lo[0], p_hi[0], zlo, zhi, w, x0, x1)
            || !cull_range(p_lo[1], p_hi[1], zlo, zhi, h, y0, y1))
            return false;
    }
    int level = 0;
    while ((x1 >> level) - (x0 >> level) > 1 || (y1 >> level) - (y0 >> level) > 1)
        ++level;
    float const inf = __builtin_huge_valf();
    float dlo = inf, dhi = -inf;
    int const wl = pyramid_side(w, level);
    const float2 *texels = P.texels + P.off[level];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        int const x = (d & 1 ? x1 : x0) >> level, y = (d >> 1 ? y1 : y0) >> level;
        if (level == 0)
            pyramid_pixel(V.depth_z[(size_t)y * w + x], dlo, dhi);
        else {
            float2 const t = texels[(size_t)y * wl + x];
            dlo = fminf(dlo, t.x);
            dhi = fmaxf(dhi, t.y);
        }
    }
    if (dlo > dhi)
        return false;
    double const znear = fmax(zlo, 0.0);
    return (double)dhi >= znear - T && (double)dlo <= zhi + T;
}

__global__ void __launch_bounds__(256)
tsdf_cull_kernel(const MeshViewDev *__restrict__ views,
    const TsdfPyramidDev *__restrict__ pyramids, TsdfGrid G, TsdfBricks B,
    uint8_t *__restrict__ candidate, unsigned long long *__restrict__ counts)
{
#pragma clang fp contract(off)
    unsigned const brick = blockIdx.x * 256u + threadIdx.x;
    bool may = false;
    if (brick < B.n) {
        int const first[3] = { (int)(brick % B.bx) * TSDF_BX, (int)(brick / B.bx % B.by) * TSDF_BY,
            (int)(brick / B.bx / B.by) * TSDF_BZ };
        int const side[3] = { TSDF_BX, TSDF_BY, TSDF_BZ }, dims[3] = { G.nx, G.ny, G.nz };
        double lo[3], hi[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            int const last = first[a] + side[a] - 1 < dims[a] - 1 ? first[a] + side[a] - 1
                                                                 : dims[a] - 1;
            lo[a] = (double)tsdf_centre(G, a, first[a]);
            hi[a] = (double)tsdf_centre(G, a, last);
        }
        double const T = (double)G.trunc * (1.0 + 0x1p-22);
        for (int v = 0; v < G.n_views && !may; ++v)
            may = cull_view(views[v], pyramids[v], lo, hi, T);
        candidate[brick] = may ? 1 : 0;
    }
    uint32_t total;
    (void)tsdf_block_scan((uint32_t)may, &total);
    if (threadIdx.x == 0)
        counts[blockIdx.x] = total;
}

__global__ void __launch_bounds__(256)
tsdf_cull_list_kernel(const uint8_t *__restrict__ candidate, TsdfBricks B,
    const unsigned long long *__restrict__ counts, uint32_t *__restrict__ list)
{
    unsigned const brick = blockIdx.x * 256u + threadIdx.x;
    bool const may = brick < B.n && candidate[brick] != 0;
    uint32_t total;
    uint32_t const before = tsdf_block_scan((uint32_t)may, &total);
    if (may)
        list[(uint32_t)counts[blockIdx.x] + before] = brick;
}

// tsdf_sparse_seed_kernel on the listed bricks
__global__ void __launch_bounds__(256)
tsdf_sparse_seed_list_kernel(const MeshViewDev *__restrict__ views, TsdfGrid G, TsdfBricks B,
    const uint32_t *__restrict__ list, unsigned n, uint8_t *__restrict__ seed)
{
#pragma clang fp contract(off)
    unsigned const at = blockIdx.y * SEED_GRID_X + blockIdx.x;
    if (at >= n)
        return;
    unsigned const brick = list[at];
    TSDF_SEED_BRICK(views, G, B, brick, seed);
}

namespace tsdf_host {

size_t
pyramid_texels(int w, int h, int *levels, uint32_t *off)
{
    size_t total = 0;
    int level = 0;
    while (w > 1 || h > 1) {
        ++level;
        w = (w + 1) / 2;
        h = (h + 1) / 2;
        if (off != nullptr)
            off[level] = (uint32_t)total;
        total += (size_t)w * h;
    }
    if (levels != nullptr)
        *levels = level;
    return total;
}

void
carve_pyramids(const smvs_point_view *views, int n_views, Carver &carve, PyramidSlab &p)
{
    p.at.resize(n_views);
    for (int i = 0; i < n_views; ++i) {
        size_t const bytes = sizeof(float2) * pyramid_texels(views[i].width, views[i].height,
            nullptr, nullptr);
        p.at[i] = carve(bytes);
        p.bytes += bytes;
        unsigned const tiles = (unsigned)((views[i].width + PYR_TILE - 1) / PYR_TILE)
            * (unsigned)((views[i].height + PYR_TILE - 1) / PYR_TILE);
        p.max_tiles = tiles > p.max_tiles ? tiles : p.max_tiles;
    }
    p.table_at = carve(sizeof(TsdfPyramidDev) * n_views);
}

int
launch_pyramids(Workspace &ws, char *slab, ViewSlab const &s, int n_views, PyramidSlab &p)
{
    int rc;
    p.table.assign(n_views, TsdfPyramidDev());
    for (int i = 0; i < n_views; ++i) {
        TsdfPyramidDev &P = p.table[i];
        P.texels = reinterpret_cast<float2 *>(slab + p.at[i]);
        for (uint32_t &o : P.off)
            o = 0;
        (void)pyramid_texels(s.table[i].w, s.table[i].h, &P.levels, P.off);
    }
    p.d_table = reinterpret_cast<TsdfPyramidDev *>(slab + p.table_at);
    if ((rc = ws.upload(p.d_table, p.table.data(), sizeof(TsdfPyramidDev) * n_views)))
        return rc;
    hipLaunchKernelGGL(tsdf_pyramid_tile_kernel, dim3(p.max_tiles, (unsigned)n_views), dim3(256),
        0, ws.stream, s.d_table, p.d_table);
    hipLaunchKernelGGL(tsdf_pyramid_top_kernel, dim3((unsigned)n_views), dim3(256), 0, ws.stream,
        s.d_table, p.d_table);
    SMVS_HIP_CHECK(hipGetLastError());
    return SMVS_OK;
}

void
launch_cull(hipStream_t stream, ViewSlab const &s, PyramidSlab const &p, TsdfGrid const &G,
    TsdfBricks const &B, uint8_t *candidate, unsigned long long *counts)
{
    hipLaunchKernelGGL(tsdf_cull_kernel, dim3((B.n + 255u) / 256u), dim3(256), 0, stream,
        s.d_table, p.d_table, G, B, candidate, counts);
}

void
launch_candidate_list(hipStream_t stream, const uint8_t *candidate, TsdfBricks const &B,
    const unsigned long long *counts, uint32_t *list)
{
    hipLaunchKernelGGL(tsdf_cull_list_kernel, dim3((B.n + 255u) / 256u), dim3(256), 0, stream,
        candidate, B, counts, list);
}

void
launch_seed_list(hipStream_t stream, ViewSlab const &s, TsdfGrid const &G, TsdfBricks const &B,
    const uint32_t *list, size_t n, uint8_t *seed)
{
    if (n == 0)
        return;
    unsigned const gx = n < SEED_GRID_X ? (unsigned)n : SEED_GRID_X;
    unsigned const gy = (unsigned)((n + SEED_GRID_X - 1) / SEED_GRID_X);
    hipLaunchKernelGGL(tsdf_sparse_seed_list_kernel, dim3(gx, gy), dim3(256), 0, stream,
        s.d_table, G, B, list, (unsigned)n, seed);
}

} // namespace tsdf_host

} // namespace smvs_hip

using namespace smvs_hip;
using namespace smvs_hip::tsdf_host;

extern "C" int
smvs_tsdf_brick_cull(int device, const smvs_point_view *views, int n_views,
    const smvs_tsdf_options *options, uint8_t *brick_candidate, int64_t *n_candidates)
{
    SMVS_REQUIRE(options != nullptr, "no options");
    SMVS_REQUIRE(brick_candidate != nullptr, "no output");
    smvs_tsdf_options const &opt = *options;
    int rc;
    if ((rc = check_views(views, n_views, opt.cut_surfaces, false)))
        return rc;
    TsdfGrid G;
    if ((rc = check_grid("smvs_tsdf_brick_cull", opt, n_views, 4096, G)))
        return rc;
    size_t n_bricks;
    TsdfBricks const B = brick_grid(G, &n_bricks);
    SMVS_REQUIRE(n_bricks <= ((size_t)1 << 28), "the brick grid has more than 2^28 bricks");

    WorkspaceLease lease(device);
    if (lease.w == nullptr)
        return SMVS_ERR_HIP;
    Workspace &ws = *lease.w;
    Carver carve;
    ViewSlab s;
    PyramidSlab pyr;
    carve_views(views, n_views, false, carve, s);
    carve_pyramids(views, n_views, carve, pyr);
    unsigned const brick_blocks = (unsigned)((n_bricks + 255) / 256);
    size_t const brick_tiles = ((size_t)brick_blocks + SCAN_TILE - 1) / SCAN_TILE;
    size_t const cand_at = carve(n_bricks), counts_at = carve(8 * (size_t)brick_blocks),
        tiles_at = carve(8 * (brick_tiles + 1));
    char *slab = nullptr;
    if ((rc = ws.ensure(0, carve.total, &slab)) != SMVS_OK)
        return rc;
    if ((rc = upload_and_prepare(ws, slab, views, n_views, opt.cut_surfaces != 0, false, s)))
        return rc;
    uint8_t *d_cand = reinterpret_cast<uint8_t *>(slab + cand_at);
    unsigned long long *d_counts = reinterpret_cast<unsigned long long *>(slab + counts_at);
    unsigned long long *d_tiles = reinterpret_cast<unsigned long long *>(slab + tiles_at);
    launch_depth(ws.stream, s, n_views);
    if ((rc = launch_pyramids(ws, slab, s, n_views, pyr)))
        return rc;
    launch_cull(ws.stream, s, pyr, G, B, d_cand, d_counts);
    SMVS_HIP_CHECK(hipGetLastError());
    if ((rc = exclusive_scan(ws.stream, d_counts, brick_blocks, d_tiles)))
        return rc;
    unsigned long long total = 0;
    if ((rc = ws.download(&total, d_tiles + brick_tiles, sizeof(total)))
        || (rc = ws.download(brick_candidate, d_cand, n_bricks)))
        return rc;
    if (n_candidates != nullptr)
        *n_candidates = (int64_t)total;
    return SMVS_OK;
}

extern "C" int
smvs_tsdf_depth_pyramid(int device, const smvs_point_view *views, int n_views, int cut_surfaces,
    int view, float *lo, float *hi, int64_t *n_texels, int *n_levels)
{
    int rc;
    if ((rc = check_views(views, n_views, cut_surfaces, false)))
        return rc;
    SMVS_REQUIRE(view >= 0 && view < n_views, "no such view");
    int levels = 0;
    size_t const texels = pyramid_texels(views[view].width, views[view].height, &levels, nullptr);
    if (n_texels != nullptr)
        *n_texels = (int64_t)texels;
    if (n_levels != nullptr)
        *n_levels = levels;
    if ((lo == nullptr && hi == nullptr) || texels == 0)
        return SMVS_OK;

    WorkspaceLease lease(device);
    if (lease.w == nullptr)
        return SMVS_ERR_HIP;
    Workspace &ws = *lease.w;
    Carver carve;
    ViewSlab s;
    PyramidSlab pyr;
    carve_views(views, n_views, false, carve, s);
    carve_pyramids(views, n_views, carve, pyr);
    char *slab = nullptr;
    if ((rc = ws.ensure(0, carve.total, &slab)) != SMVS_OK)
        return rc;
    if ((rc = upload_and_prepare(ws, slab, views, n_views, cut_surfaces != 0, false, s)))
        return rc;
    launch_depth(ws.stream, s, n_views);
    if ((rc = launch_pyramids(ws, slab, s, n_views, pyr)))
        return rc;
    std::vector<float2> host(texels);
    if ((rc = ws.download(host.data(), pyr.table[view].texels, sizeof(float2) * texels)))
        return rc;
    for (size_t e = 0; e < texels; ++e) {
        if (lo != nullptr)
            lo[e] = host[e].x;
        if (hi != nullptr)
            hi[e] = host[e].y;
    }
    return SMVS_OK;
}
