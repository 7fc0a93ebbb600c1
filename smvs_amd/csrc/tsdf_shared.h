// Pieces of the volumetric fusion that tsdf.hip (the dense volume),
// tsdf_sparse.hip (the brick-sparse volume), tsdf_cull.hip (the brick cull
// in front of its seed pass), tsdf_volume.hip (the persistent dense volume)
// and tsdf_volume_sparse.hip (the persistent brick-sparse volume) share: the
// grid record, the brick grid, the
// per-element device functions of the definition in include/smvs_hip.h (voxel
// centre, the projection steps 1-6, the cell / edge / quad rules, the block
// scan, the vertex attribute arithmetic) and the host pieces of the entries.
// The field functions take the field as (pointer, grid): tsdf.hip hands them
// the volume, tsdf_sparse.hip a brick with its halo staged in LDS.
#pragma once

#include "common.h"
#include "export_shared.h"
#include "mesh_shared.h"

#include <vector>

namespace smvs_hip {

struct TsdfGrid {
    int nx, ny, nz;
    float origin[3];
    float voxel_size, trunc;
    uint32_t min_weight;
    int n_views;
};

struct TsdfImageDev {
    const uint8_t *image;   // w * h * channels
    int channels;
};

// A block is a brick of 8 x 8 x 4 voxels (a wave is one 8 x 8 slab of it), so
// that the 64 gathers of a wave land in a small patch of each depth map.
constexpr int TSDF_BX = 8, TSDF_BY = 8, TSDF_BZ = 4;

// the centre of voxel (or grid point) idx along one axis
__device__ __forceinline__ float
tsdf_centre(TsdfGrid const &G, int axis, int idx)
{
#pragma clang fp contract(off)
    return G.origin[axis] + ((float)idx + 0.5f) * G.voxel_size;
}

// Two pieces are macros, not functions: behind a function boundary the compiler
// gives tsdf_integrate_kernel and tsdf_vertex_kernel other registers and another
// schedule than they had with the text in their bodies (tools/
// kernel_isa_diff.py; profiles/tsdf_sparse_kernel_resources.txt), and those
// kernels keep the code they were measured with.  The text exists once.
//
// Field, steps 1-6 for the view V and the voxel centre c, inside a scope with
// `#pragma clang fp contract(off)`: declares pj (the pixel) and sdf, or leaves
// through SKIP (`continue`, `return false`)
#define TSDF_STEPS_1_TO_6(V, c, trunc, SKIP)                                     \
    float proj[3];                                                             \
    proj[0] = dot3((V).KR + 0, c) - (V).t[0];                                  \
    proj[1] = dot3((V).KR + 3, c) - (V).t[1];                                  \
    proj[2] = dot3((V).KR + 6, c) - (V).t[2];                                  \
    if (proj[2] <= 0.0f)                                                       \
        SKIP;                                                                  \
    float const u = proj[0] / proj[2];                                         \
    float const w = proj[1] / proj[2];                                         \
    if (u < 0.0f || w < 0.0f)                                                  \
        SKIP;                                                                  \
    int const xj = (int)u;                                                     \
    int const yj = (int)w;                                                     \
    if (xj >= (V).w || yj >= (V).h)                                            \
        SKIP;                                                                  \
    size_t const pj = (size_t)yj * (V).w + xj;                                 \
    float const D = (V).depth_z[pj];                                           \
    if (D == 0.0f)                                                             \
        SKIP;                                                                  \
    float const sdf = D - proj[2];                                             \
    if (sdf < -(trunc))                                                        \
        SKIP

// steps 1-6 as a function: false where the view is skipped, else the pixel the
// voxel centre falls into and its signed distance
__device__ __forceinline__ bool
tsdf_project(MeshViewDev const &V, const float *c, float trunc, size_t *pixel, float *sdf_out)
{
#pragma clang fp contract(off)
    TSDF_STEPS_1_TO_6(V, c, trunc, return false);
    *pixel = pj;
    *sdf_out = sdf;
    return true;
}

// ---------------------------------------------------------------- brick grid
// tsdf_sparse.hip and tsdf_cull.hip: the bricks of the whole grid
struct TsdfBricks {
    int bx, by, bz;
    unsigned n;      // bx * by * bz <= 2^28
};

// (a launch's x extent in threads is 32 bits: a block per brick goes over x and y)
constexpr unsigned SEED_GRID_X = 65536;

struct BrickVoxel {
    int i, j, k;       // the voxel in the grid
    bool in_grid;
};

__device__ __forceinline__ BrickVoxel
brick_voxel(TsdfGrid const &G, TsdfBricks const &B, unsigned brick)
{
    BrickVoxel v;
    v.i = (int)(brick % B.bx) * TSDF_BX + (int)(threadIdx.x & 7);
    v.j = (int)(brick / B.bx % B.by) * TSDF_BY + (int)(threadIdx.x >> 3 & 7);
    v.k = (int)(brick / B.bx / B.by) * TSDF_BZ + (int)(threadIdx.x >> 6);
    v.in_grid = v.i < G.nx && v.j < G.ny && v.k < G.nz;
    return v;
}

// The exact seed test of one brick by its block of 256 (a macro: see above;
// tsdf_sparse_seed_kernel keeps its code): seed[brick] = 2 where a voxel of
// the brick has C > 0, else 0.  Inside a scope with
// `#pragma clang fp contract(off)`; every thread of the block runs it.
#define TSDF_SEED_BRICK(views, G, B, brick, seed)                                \
    __shared__ uint32_t found;                                                 \
    if (threadIdx.x == 0)                                                      \
        found = 0;                                                             \
    __syncthreads();                                                           \
    BrickVoxel const p = brick_voxel(G, B, brick);                             \
    float const c[3] = { tsdf_centre(G, 0, p.i), tsdf_centre(G, 1, p.j),       \
        tsdf_centre(G, 2, p.k) };                                              \
    for (int v = 0; v < (G).n_views; ++v) {                                    \
        /* another wave's hit ends this wave too */                            \
        if (__builtin_amdgcn_readfirstlane(*(volatile uint32_t *)&found) != 0) \
            break;                                                             \
        bool hit = false;                                                      \
        if (p.in_grid) {                                                       \
            size_t pj;                                                         \
            float sdf;                                                         \
            hit = tsdf_project((views)[v], c, (G).trunc, &pj, &sdf) && sdf <= (G).trunc; \
        }                                                                      \
        if (__ballot(hit) != 0) {                                              \
            if ((threadIdx.x & 63) == 0)                                       \
                *(volatile uint32_t *)&found = 1;                              \
            break;                                                             \
        }                                                                      \
    }                                                                          \
    __syncthreads();                                                           \
    if (threadIdx.x == 0)                                                      \
        (seed)[brick] = found != 0 ? 2 : 0

// ------------------------------------------------------------ cull (9.10)
// One view's min/max pyramid of D, levels 1 .. levels (level 0 is depth_z
// itself): texel (x, y) of level l is texels[off[l] + y * w_l + x] = (lo, hi),
// w_l = ceil(w / 2^l); (+inf, -inf) where no pixel below it is valid
constexpr int TSDF_PYRAMID_MAX_LEVELS = 31;
struct TsdfPyramidDev {
    float2 *texels;
    int levels;
    uint32_t off[TSDF_PYRAMID_MAX_LEVELS + 1];
};

// ----------------------------------------------------------------- extraction
// Cells and grid points share the points' linear index (x fastest): cell
// (i, j, k) is the one whose corner 0 is point (i, j, k).

__device__ __forceinline__ size_t
tsdf_index(TsdfGrid const &G, int i, int j, int k)
{
    return ((size_t)k * G.ny + j) * G.nx + i;
}

// the cell's corners c = dx + 2 dy + 4 dz; -> complete (in the grid, no NaN)
__device__ __forceinline__ bool
tsdf_cell(const float *__restrict__ tsdf, TsdfGrid const &G, int i, int j, int k, float *f)
{
    if (i < 0 || j < 0 || k < 0 || i > G.nx - 2 || j > G.ny - 2 || k > G.nz - 2)
        return false;
    bool complete = true;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        f[c] = tsdf[tsdf_index(G, i + (c & 1), j + (c >> 1 & 1), k + (c >> 2))];
        complete = complete && !(f[c] != f[c]);
    }
    return complete;
}

__device__ __forceinline__ bool
tsdf_cell_active(const float *__restrict__ tsdf, TsdfGrid const &G, int i, int j, int k,
    float *f)
{
    if (!tsdf_cell(tsdf, G, i, j, k, f))
        return false;
    int inside = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c)
        inside += f[c] < 0.0f;
    return inside != 0 && inside != 8;
}

// the four cells around the edge from point (i, j, k) along axis a, as (b, c)
// offsets with (a, b, c) cyclic: (-1,-1) (0,-1) (0,0) (-1,0)
__device__ __forceinline__ void
tsdf_quad_cell(int a, int q, int i, int j, int k, int *cell)
{
    int const ob = (q == 1 || q == 2) ? 0 : -1;
    int const oc = (q == 2 || q == 3) ? 0 : -1;
    int off[3] = { 0, 0, 0 };
    off[(a + 1) % 3] = ob;
    off[(a + 2) % 3] = oc;
    cell[0] = i + off[0];
    cell[1] = j + off[1];
    cell[2] = k + off[2];
}

// Faces: bit a set when the edge along axis a has a quad; bit 3: P is inside
__device__ __forceinline__ int
tsdf_quads(const float *__restrict__ tsdf, TsdfGrid const &G, int i, int j, int k)
{
    int const n[3] = { G.nx, G.ny, G.nz };
    int const p[3] = { i, j, k };
    float const fa = tsdf[tsdf_index(G, i, j, k)];
    if (fa != fa)
        return 0;
    int mask = fa < 0.0f ? 8 : 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (p[a] > n[a] - 2)
            continue;
        float const fb = tsdf[tsdf_index(G, i + (a == 0), j + (a == 1), k + (a == 2))];
        if (fb != fb || (fa < 0.0f) == (fb < 0.0f))
            continue;
        bool all = true;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (!all)
                break;
            int cell[3];
            float f[8];
            tsdf_quad_cell(a, q, i, j, k, cell);
            all = tsdf_cell(tsdf, G, cell[0], cell[1], cell[2], f);
        }
        if (all)
            mask |= 1 << a;
    }
    return mask;
}

// exclusive scan of one 32-bit value per thread over the block of 256 and the
// block's total; every thread of the block calls it
__device__ __forceinline__ uint32_t
tsdf_block_scan(uint32_t v, uint32_t *total)
{
    __shared__ uint32_t wsum[4];
    int const lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        uint32_t const t = __shfl_up(inc, o, 64);
        if (lane >= o)
            inc += t;
    }
    if (lane == 63)
        wsum[wave] = inc;
    __syncthreads();
    uint32_t pre = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        pre += w < wave ? wsum[w] : 0u;
        tot += wsum[w];
    }
    __syncthreads();
    *total = tot;
    return pre + inc - v;
}

// per thread: active cell (0 / 1) | quads (0..3) << 16, each where asked for
template <bool CELLS, bool QUADS>
__device__ __forceinline__ uint32_t
tsdf_classify(const float *__restrict__ tsdf, TsdfGrid const &G, bool valid, int i, int j,
    int k, float *f, bool *active, int *quads)
{
    *active = false;
    *quads = 0;
    if (!valid)
        return 0;
    if constexpr (CELLS)
        *active = tsdf_cell_active(tsdf, G, i, j, k, f);
    if constexpr (QUADS)
        *quads = tsdf_quads(tsdf, G, i, j, k);
    return (uint32_t)*active | (uint32_t)__popc(*quads & 7) << 16;
}

struct TsdfOut {
    float *xyz, *nrm, *conf;
    uint8_t *rgb;
    uint32_t *faces;
};

// Vertices: position and normal of the active cell `cell` (int[3], indices in
// the grid G) with the corner values f, written at rank id; inside a scope
// with `#pragma clang fp contract(off)` (a macro: see above).  Edges in the
// definition's order: x (0,1) (2,3) (4,5) (6,7), y (0,2) (1,3) (4,6) (5,7),
// z (0,4) (1,5) (2,6) (3,7); the two axes other than `axis`, lower first,
// carry e's bits.
#define TSDF_VERTEX_GEOMETRY(G, cell, f, id, O)                                  \
    float sum[3] = { 0.0f, 0.0f, 0.0f }, g[3] = { 0.0f, 0.0f, 0.0f };          \
    int m = 0;                                                                 \
    _Pragma("unroll")                                                          \
    for (int axis = 0; axis < 3; ++axis) {                                     \
        _Pragma("unroll")                                                      \
        for (int e = 0; e < 4; ++e) {                                          \
            int const lo_axis = axis == 0 ? 1 : 0, hi_axis = axis == 2 ? 1 : 2; \
            int const a = (e & 1) << lo_axis | (e >> 1) << hi_axis;            \
            int const b = a | 1 << axis;                                       \
            g[axis] += f[b] - f[a];                                            \
            if ((f[a] < 0.0f) == (f[b] < 0.0f))                                \
                continue;                                                      \
            float const t = f[a] / (f[a] - f[b]);                              \
            float q[3];                                                        \
            _Pragma("unroll")                                                  \
            for (int r = 0; r < 3; ++r)                                        \
                q[r] = tsdf_centre(G, r, cell[r] + (a >> r & 1));              \
            q[axis] = q[axis] + t * (G).voxel_size;                            \
            _Pragma("unroll")                                                  \
            for (int r = 0; r < 3; ++r)                                        \
                sum[r] += q[r];                                                \
            ++m;                                                               \
        }                                                                      \
    }                                                                          \
    for (int r = 0; r < 3; ++r)                                                \
        (O).xyz[3 * (id) + r] = sum[r] / (float)m;                             \
    float const len = sqrtf(dot3(g, g));                                       \
    for (int r = 0; r < 3; ++r)                                                \
        (O).nrm[3 * (id) + r] = len == 0.0f ? 0.0f : g[r] / len

// Vertices: colour and confidence from the sums over the cell's 8 corners (a
// macro: see above)
#define TSDF_VERTEX_ATTRIBUTES(G, Rs, Gs, Bs, Cs, Ws, id, O)                     \
    (O).rgb[3 * (id) + 0] = Cs == 0 ? 0 : (uint8_t)((2 * Rs + Cs) / (2 * Cs)); \
    (O).rgb[3 * (id) + 1] = Cs == 0 ? 0 : (uint8_t)((2 * Gs + Cs) / (2 * Cs)); \
    (O).rgb[3 * (id) + 2] = Cs == 0 ? 0 : (uint8_t)((2 * Bs + Cs) / (2 * Cs)); \
    (O).conf[id] = (float)Ws / (float)(8 * (G).n_views)

// Faces: the two triangles of a quad with the corners v0 .. v3
__device__ __forceinline__ void
tsdf_quad_faces(const uint32_t *v, bool inside, uint32_t *out)
{
    out[0] = v[0];
    out[1] = inside ? v[1] : v[2];
    out[2] = inside ? v[2] : v[1];
    out[3] = v[0];
    out[4] = inside ? v[2] : v[3];
    out[5] = inside ? v[3] : v[2];
}

// ----------------------------------------------------------------------- host
// tsdf.hip: what the entries share on top of the view stage (export_shared.h:
// carve_views / upload_and_prepare lay the views' maps out, upload, prepare
// and cut them as every export path does)
namespace tsdf_host {

// The limits of the entries.  TSDF_MAX_VOXELS: the dense volume's size
// (smvs_tsdf_fuse, smvs_tsdf_volume_create), and the grid up to which the
// brick-sparse entries hand tsdf / weight out
constexpr size_t TSDF_MAX_VOXELS = (size_t)1 << 27;
constexpr size_t MAX_BRICKS_GRID = (size_t)1 << 28;
constexpr int64_t DEFAULT_MAX_BRICKS = (int64_t)1 << 20;
constexpr int64_t MAX_MAX_BRICKS = (int64_t)1 << 23;       // vertex ids are 32 bits
// what the stats and the budget's text count per allocated brick: the
// one-shot entry's 24 bytes of sums and 4 of vertex id per voxel, the volume's
// sums alone (its vertex ids live in a workspace for the length of an extract)
constexpr int64_t ONE_SHOT_STATE_BYTES_PER_BRICK = 256 * 28;
constexpr int64_t VOLUME_STATE_BYTES_PER_BRICK = 256 * 24;
// a persistent volume: 255 * n_views must fit uint32 (the colour sums),
// 8 * n_views an int (the confidence's divisor)
constexpr int64_t VOLUME_MAX_VIEWS = (int64_t)1 << 24;

// argument checks shared by the entries (before any device call)
int check_views(const smvs_point_view *views, int n_views, int cut, bool want_images);
// smvs_tsdf_options with each dim 2 .. max_dim (1024 or 4096); fills the grid record
// (`who` heads the error text)
int check_grid(const char *who, const smvs_tsdf_options &opt, int n_views, int max_dim,
    TsdfGrid &G);
// check_grid on a volume's options record (smvs_tsdf_volume_options,
// smvs_tsdf_sparse_volume_options): a grid without a view list
template <class VolumeOptions> int
check_volume_grid(const char *who, VolumeOptions const &options, int max_dim, TsdfGrid &G)
{
    smvs_tsdf_options opt = {};
    for (int r = 0; r < 3; ++r) {
        opt.origin[r] = options.origin[r];
        opt.dims[r] = options.dims[r];
    }
    opt.voxel_size = options.voxel_size;
    opt.trunc = options.trunc;
    return check_grid(who, opt, 0, max_dim, G);
}
// the fusing entries' colour table, n_views records at slab + at, from the
// images the view stage uploaded
int upload_image_table(Workspace &ws, char *slab, size_t at, const smvs_point_view *views,
    ViewSlab const &s, TsdfImageDev **d_images);
// D(p) = depth_z[p] where cut[p] != 0, else 0, in place in depth_z
void launch_depth(hipStream_t stream, ViewSlab const &s, int n_views);
// The staging of a view list, as every entry that walks one does it: the view
// stage's pieces are carved first (and the colour table's with want_images),
// then the caller's own (`more(carve)`), all in the slab of slot 0; the views
// are uploaded, prepared and cut, the colour table uploaded, and D launched.
struct ViewStage {
    Carver carve;
    ViewSlab s;
    char *slab = nullptr;
    TsdfImageDev *d_images = nullptr;    // with want_images

    template <class More> int
    operator()(Workspace &ws, const smvs_point_view *views, int n_views, bool cut,
        bool want_images, More more)
    {
        carve_views(views, n_views, want_images, carve, s);
        size_t const images_at = want_images ? carve(sizeof(TsdfImageDev) * n_views) : 0;
        more(carve);
        int rc;
        if ((rc = ws.ensure(0, carve.total, &slab)) != SMVS_OK)
            return rc;
        if ((rc = upload_and_prepare(ws, slab, views, n_views, cut, want_images, s))
            || (want_images && (rc = upload_image_table(ws, slab, images_at, views, s, &d_images))))
            return rc;
        launch_depth(ws.stream, s, n_views);
        return SMVS_OK;
    }
};
// a finished mesh goes out: the entries' last step
inline int
publish(smvs_points *h, smvs_points **handle, int64_t *n_vertices, int64_t *n_faces)
{
    *handle = h;
    if (n_vertices != nullptr)
        *n_vertices = h->n_points;
    if (n_faces != nullptr)
        *n_faces = h->n_faces;
    return SMVS_OK;
}
// The extraction half of smvs_tsdf_fuse, which smvs_tsdf_volume_extract
// (tsdf_volume.hip) runs as well: classify, scan, vertices, faces, fill on a
// field, weights and colour sums that are on the device (x fastest).
// carve_extract lays its work arrays (cell -> vertex id, block counts, scan
// tiles) out in the slab of slot 0; the vertices and faces go to slot 1.
struct ExtractPieces {
    size_t vid, counts, tiles;   // offsets in the slab
    unsigned point_blocks;
};
void carve_extract(size_t n_vox, Carver &carve, ExtractPieces &at);
// G.n_views is the confidence's view count; `who` heads the error text.  On
// failure no handle is left behind.
int extract_surface(Workspace &ws, const char *who, TsdfGrid const &G, char *slab,
    ExtractPieces const &at, const float *d_tsdf, const uint32_t *d_weight,
    const uint4 *d_colour, smvs_points **handle);

// tsdf_cull.hip: the views' pyramids in the same slab and the passes over them
struct PyramidSlab {
    std::vector<size_t> at;              // per view: its texels
    std::vector<TsdfPyramidDev> table;
    size_t table_at = 0, bytes = 0;      // bytes: all views' texels
    unsigned max_tiles = 0;
    TsdfPyramidDev *d_table = nullptr;
};
// levels and the texels of levels >= 1 of a w x h map; off (may be null): the
// TsdfPyramidDev offsets
size_t pyramid_texels(int w, int h, int *levels, uint32_t *off);
void carve_pyramids(const smvs_point_view *views, int n_views, Carver &carve, PyramidSlab &p);
// after launch_depth: uploads the table and builds every view's levels
int launch_pyramids(Workspace &ws, char *slab, ViewSlab const &s, int n_views, PyramidSlab &p);
// candidate[brick] = 0 / 1 and counts[block of 256 bricks] = its candidates
void launch_cull(hipStream_t stream, ViewSlab const &s, PyramidSlab const &p, TsdfGrid const &G,
    TsdfBricks const &B, uint8_t *candidate, unsigned long long *counts);
// counts scanned: list[rank] = brick for the candidates in brick order
void launch_candidate_list(hipStream_t stream, const uint8_t *candidate, TsdfBricks const &B,
    const unsigned long long *counts, uint32_t *list);
// the exact seed test on the n bricks of the list; the other bytes are not written
void launch_seed_list(hipStream_t stream, ViewSlab const &s, TsdfGrid const &G,
    TsdfBricks const &B, const uint32_t *list, size_t n, uint8_t *seed);
// the entry behind smvs_tsdf_fuse_sparse and smvs_tsdf_fuse_sparse_opts (tsdf_sparse.hip)
TsdfBricks brick_grid(TsdfGrid const &G, size_t *n_bricks);

// tsdf_sparse.hip: the passes of smvs_tsdf_fuse_sparse_opts that the persistent
// brick-sparse volume (tsdf_volume_sparse.hip) runs as well.
// Their work arrays over the bricks of the grid, in a ViewStage's slab: the
// seed and state bytes, the table (whose place holds the cull's candidate list
// first), the counts per 256 bricks and their scan's tiles; with the cull the
// views' pyramids and the candidate bytes behind them.
struct BrickWork {
    bool cull = false;
    unsigned blocks = 0;        // of 256 bricks
    PyramidSlab pyr;
    uint8_t *seed = nullptr, *state = nullptr, *cand = nullptr;
    int32_t *table = nullptr;
    unsigned long long *counts = nullptr, *tiles = nullptr;

    void carve(const smvs_point_view *views, int n_views, size_t n_bricks, bool with_cull,
        Carver &carve);
    void place(char *slab);     // the pointers, once the slab is there
private:
    size_t seed_at = 0, state_at = 0, table_at = 0, counts_at = 0, tiles_at = 0, cand_at = 0;
};
// After launch_depth: the list's seed bytes (2 / 0 per brick) in w.seed.
// Without w.cull the exact test on every brick.  Else the cull in front
// (launch_pyramids, launch_cull, the candidates' list, the exact test on the
// list).  brick_candidate (host, may be null) and *n_tested as
// smvs_tsdf_fuse_sparse_opts gives them.
int launch_seeds(Workspace &ws, char *slab, ViewSlab const &s, int n_views, TsdfGrid const &G,
    TsdfBricks const &B, BrickWork &w, uint8_t *brick_candidate, size_t *n_tested);
// state[brick] = 2 seed, 1 a neighbour of a seed, 0 neither; counts[block of 256
// bricks] = allocated | seeds << 32
void launch_dilate(hipStream_t stream, const uint8_t *seed, TsdfBricks const &B, uint8_t *state,
    unsigned long long *counts);
// counts scanned: brick -> slot (or -1) and slot -> brick, in linear brick order
void launch_table(hipStream_t stream, const uint8_t *state, TsdfBricks const &B,
    const unsigned long long *counts, int32_t *table, uint32_t *list);
// The extraction half of smvs_tsdf_fuse_sparse_opts, which
// smvs_tsdf_sparse_volume_extract runs as well: classify, scan, vertices, faces
// and fill on a slot-major field, weights and colour sums, a table and a list
// (slots in linear brick order) that are on the device, then tsdf / weight
// (host, either may be null) as the whole grid.  Work arrays go to slot 3 of
// the workspace, vertices and faces to slot 1.  G.n_views is the confidence's
// view count; `who` heads the error text.  On failure no handle is left behind.
int extract_sparse_surface(Workspace &ws, const char *who, TsdfGrid const &G,
    TsdfBricks const &B, size_t n_alloc, const float *d_tsdf, const uint32_t *d_weight,
    const uint4 *d_colour, const int32_t *d_table, const uint32_t *d_list, float *tsdf,
    uint32_t *weight, smvs_points **handle);

} // namespace tsdf_host

} // namespace smvs_hip
