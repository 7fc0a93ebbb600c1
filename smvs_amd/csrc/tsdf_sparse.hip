// Volumetric fusion on a brick-sparse volume on gfx950 (DESIGN.md section 9.9;
// opt-in).  The normative definition is the comment of smvs_tsdf_fuse_sparse in
// include/smvs_hip.h, restated by tests/tsdf_sparse_ref.py: the field, the
// vertices and the faces are smvs_tsdf_fuse's (tsdf_shared.h), computed only in
// the 8 x 8 x 4 bricks that hold a voxel within the truncation band of some view
// or touch a brick that does.
//   seed       one block per brick of the whole grid runs steps 1-6 and the
//              test of step 8 until the first hit: one byte per brick (with
//              the cull of tsdf_cull.hip, section 9.10: per candidate brick)
//   dilate     per brick the OR over its 27 neighbours; counts per 256 bricks
//   scan       export_common.hip's exclusive_scan over those counts
//   table      brick -> slot (or -1) and slot -> brick, in linear brick order
//   integrate  one block per allocated brick, state slot-major (slot * 256 +
//              the voxel's index in the brick)
//   classify, scan, vertices, faces per allocated brick: a block stages its
//              brick's F with a one-voxel halo in LDS through the table and
//              classifies from LDS alone
// Arithmetic: float, FMA contraction off.  No atomics: every order is an index
// order.  A block of the seed pass ends early through one LDS word that only
// ever goes from 0 to 1; the byte it writes is the OR either way.
#include "common.h"
#include "mesh_shared.h"
#include "tsdf_shared.h"

#include <cmath>
#include <vector>

namespace smvs_hip {

// the halo of a brick as a grid of its own: the shared cell and quad rules
// read it as they read the dense volume
constexpr int HALO_X = TSDF_BX + 2, HALO_Y = TSDF_BY + 2, HALO_Z = TSDF_BZ + 2;
constexpr int HALO_N = HALO_X * HALO_Y * HALO_Z;

// where voxel (i, j, k) of the grid lives in the slot-major state; false where
// its brick is not allocated
__device__ __forceinline__ bool
sparse_at(TsdfBricks const &B, const int32_t *__restrict__ table, int i, int j, int k,
    size_t *at)
{
    unsigned const brick = ((unsigned)(k / TSDF_BZ) * B.by + (unsigned)(j / TSDF_BY)) * B.bx
        + (unsigned)(i / TSDF_BX);
    int32_t const slot = table[brick];
    if (slot < 0)
        return false;
    *at = (size_t)slot * 256
        + (size_t)(((k % TSDF_BZ) * TSDF_BY + (j % TSDF_BY)) * TSDF_BX + (i % TSDF_BX));
    return true;
}

// Seed: does the brick hold a voxel with C > 0 (some view passes steps 1-6 and
// has sdf <= trunc)?  state[brick] = 2 or 0.
__global__ void __launch_bounds__(256)
tsdf_sparse_seed_kernel(const MeshViewDev *__restrict__ views, TsdfGrid G, TsdfBricks B,
    uint8_t *__restrict__ seed)
{
#pragma clang fp contract(off)
    unsigned const brick = blockIdx.y * SEED_GRID_X + blockIdx.x;
    if (brick >= B.n)
        return;
    TSDF_SEED_BRICK(views, G, B, brick, seed);
}

// Dilate and count: state = 2 seed, 1 a neighbour of a seed, 0 neither;
// counts[block] = allocated | seeds << 32 over the block's 256 bricks
__global__ void __launch_bounds__(256)
tsdf_sparse_dilate_kernel(const uint8_t *__restrict__ seed, TsdfBricks B,
    uint8_t *__restrict__ state, unsigned long long *__restrict__ counts)
{
    unsigned const brick = blockIdx.x * 256u + threadIdx.x;
    bool const valid = brick < B.n;
    uint32_t mine = 0;
    if (valid) {
        int const bi = (int)(brick % B.bx), bj = (int)(brick / B.bx % B.by),
            bk = (int)(brick / B.bx / B.by);
        bool const own = seed[brick] == 2;
        bool any = false;
        for (int dk = -1; dk <= 1; ++dk)
            for (int dj = -1; dj <= 1; ++dj)
                for (int di = -1; di <= 1; ++di) {
                    int const ni = bi + di, nj = bj + dj, nk = bk + dk;
                    if (ni < 0 || nj < 0 || nk < 0 || ni >= B.bx || nj >= B.by || nk >= B.bz)
                        continue;
                    any = any || seed[((unsigned)nk * B.by + nj) * B.bx + ni] == 2;
                }
        state[brick] = own ? 2 : (any ? 1 : 0);
        mine = (uint32_t)any | (uint32_t)own << 16;
    }
    uint32_t total;
    (void)tsdf_block_scan(mine, &total);
    if (threadIdx.x == 0)
        counts[blockIdx.x] = (unsigned long long)(total & 0xffffu)
            | (unsigned long long)(total >> 16) << 32;
}

// the brick table and the slot -> brick list from the scanned counts
__global__ void __launch_bounds__(256)
tsdf_sparse_table_kernel(const uint8_t *__restrict__ state, TsdfBricks B,
    const unsigned long long *__restrict__ counts, int32_t *__restrict__ table,
    uint32_t *__restrict__ list)
{
    unsigned const brick = blockIdx.x * 256u + threadIdx.x;
    bool const valid = brick < B.n;
    bool const allocated = valid && state[brick] != 0;
    uint32_t total;
    uint32_t const before = tsdf_block_scan((uint32_t)allocated, &total);
    if (!valid)
        return;
    uint32_t const slot = (uint32_t)counts[blockIdx.x] + before;
    table[brick] = allocated ? (int32_t)slot : -1;
    if (allocated)
        list[slot] = brick;
}

// Field, steps 1-8 and the division after the loop, for the voxels of one
// allocated brick (tsdf_integrate_kernel's arithmetic)
__global__ void __launch_bounds__(256)
tsdf_sparse_integrate_kernel(const MeshViewDev *__restrict__ views,
    const TsdfImageDev *__restrict__ images, TsdfGrid G, TsdfBricks B,
    const uint32_t *__restrict__ list, float *__restrict__ tsdf, uint32_t *__restrict__ weight,
    uint4 *__restrict__ colour)
{
#pragma clang fp contract(off)
    BrickVoxel const p = brick_voxel(G, B, list[blockIdx.x]);
    size_t const at = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (!p.in_grid) {
        tsdf[at] = __builtin_nanf("");
        weight[at] = 0;
        colour[at] = make_uint4(0, 0, 0, 0);
        return;
    }
    float const c[3] = { tsdf_centre(G, 0, p.i), tsdf_centre(G, 1, p.j), tsdf_centre(G, 2, p.k) };
    float S = 0.0f;
    uint32_t W = 0, R = 0, Gr = 0, Bl = 0, C = 0;
    for (int v = 0; v < G.n_views; ++v) {
        size_t pj;
        float sdf;
        if (!tsdf_project(views[v], c, G.trunc, &pj, &sdf))
            continue;
        S += fminf(1.0f, sdf / G.trunc);
        W += 1;
        if (sdf <= G.trunc) {
            int const ch = images[v].channels;
            const uint8_t *px = images[v].image + pj * ch;
            uint32_t const g = px[0];
            R += g;
            Gr += ch >= 3 ? px[1] : g;
            Bl += ch >= 3 ? px[2] : g;
            C += 1;
        }
    }
    tsdf[at] = W >= G.min_weight ? S / (float)W : __builtin_nanf("");
    weight[at] = W;
    colour[at] = make_uint4(R, Gr, Bl, C);
}

// ----------------------------------------------------------------- extraction
// F of the brick of block `slot` with a one-voxel halo, through the table: NaN
// outside the grid and where the neighbour brick is not allocated.  Every
// thread of the block calls it; -> this thread's voxel
__device__ __forceinline__ BrickVoxel
sparse_stage(const float *__restrict__ tsdf, const int32_t *__restrict__ table,
    const uint32_t *__restrict__ list, TsdfGrid const &G, TsdfBricks const &B, float *halo)
{
    unsigned const brick = list[blockIdx.x];
    int const i0 = (int)(brick % B.bx) * TSDF_BX - 1, j0 = (int)(brick / B.bx % B.by) * TSDF_BY - 1,
        k0 = (int)(brick / B.bx / B.by) * TSDF_BZ - 1;
    for (int e = threadIdx.x; e < HALO_N; e += 256) {
        int const i = i0 + e % HALO_X, j = j0 + e / HALO_X % HALO_Y, k = k0 + e / (HALO_X * HALO_Y);
        float f = __builtin_nanf("");
        size_t at;
        if (i >= 0 && j >= 0 && k >= 0 && i < G.nx && j < G.ny && k < G.nz
            && sparse_at(B, table, i, j, k, &at))
            f = tsdf[at];
        halo[e] = f;
    }
    __syncthreads();
    return brick_voxel(G, B, brick);
}

__device__ __forceinline__ TsdfGrid
halo_grid()
{
    TsdfGrid H = {};
    H.nx = HALO_X;
    H.ny = HALO_Y;
    H.nz = HALO_Z;
    return H;
}

// this thread's point inside the halo grid
#define SPARSE_LOCAL                                                             \
    int const li = (int)(threadIdx.x & 7) + 1, lj = (int)(threadIdx.x >> 3 & 7) + 1, \
        lk = (int)(threadIdx.x >> 6) + 1

__global__ void __launch_bounds__(256)
tsdf_sparse_classify_kernel(const float *__restrict__ tsdf, const int32_t *__restrict__ table,
    const uint32_t *__restrict__ list, TsdfGrid G, TsdfBricks B,
    unsigned long long *__restrict__ counts)
{
    __shared__ float halo[HALO_N];
    (void)sparse_stage(tsdf, table, list, G, B, halo);
    TsdfGrid const H = halo_grid();
    SPARSE_LOCAL;
    int quads;
    bool active;
    float f[8];
    uint32_t const mine = tsdf_classify<true, true>(halo, H, true, li, lj, lk, f, &active, &quads);
    uint32_t total;
    (void)tsdf_block_scan(mine, &total);
    if (threadIdx.x == 0)
        counts[blockIdx.x] = (unsigned long long)(total & 0xffffu)
            | (unsigned long long)(total >> 16) << 32;
}

// Vertices: as tsdf_vertex_kernel, at the rank in (slot, index in the brick);
// cell[id] = the cell's linear index in the whole grid
__global__ void __launch_bounds__(256)
tsdf_sparse_vertex_kernel(const float *__restrict__ tsdf, const uint32_t *__restrict__ weight,
    const uint4 *__restrict__ colour, const int32_t *__restrict__ table,
    const uint32_t *__restrict__ list, TsdfGrid G, TsdfBricks B,
    const unsigned long long *__restrict__ counts, uint32_t *__restrict__ vid, TsdfOut O,
    long long *__restrict__ cells)
{
#pragma clang fp contract(off)
    __shared__ float halo[HALO_N];
    BrickVoxel const p = sparse_stage(tsdf, table, list, G, B, halo);
    TsdfGrid const H = halo_grid();
    SPARSE_LOCAL;
    int quads;
    bool active;
    float f[8];
    uint32_t const mine = tsdf_classify<true, false>(halo, H, true, li, lj, lk, f, &active, &quads);
    uint32_t total;
    uint32_t const before = tsdf_block_scan(mine, &total);
    if (!active)
        return;
    size_t const id = (size_t)(uint32_t)counts[blockIdx.x] + (before & 0xffffu);
    vid[(size_t)blockIdx.x * 256 + threadIdx.x] = (uint32_t)id;
    cells[id] = (long long)tsdf_index(G, p.i, p.j, p.k);
    int const cell[3] = { p.i, p.j, p.k };
    TSDF_VERTEX_GEOMETRY(G, cell, f, id, O);
    uint32_t Rs = 0, Gs = 0, Bs = 0, Cs = 0, Ws = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        // the corners of an active cell are known: their bricks are allocated
        size_t at;
        if (!sparse_at(B, table, p.i + (c & 1), p.j + (c >> 1 & 1), p.k + (c >> 2), &at))
            continue;
        uint4 const col = colour[at];
        Rs += col.x;
        Gs += col.y;
        Bs += col.z;
        Cs += col.w;
        Ws += weight[at];
    }
    TSDF_VERTEX_ATTRIBUTES(G, Rs, Gs, Bs, Cs, Ws, id, O);
}

// Faces: as tsdf_face_kernel, the grid points in (slot, index in the brick) order
__global__ void __launch_bounds__(256)
tsdf_sparse_face_kernel(const float *__restrict__ tsdf, const int32_t *__restrict__ table,
    const uint32_t *__restrict__ list, TsdfGrid G, TsdfBricks B,
    const unsigned long long *__restrict__ counts, const uint32_t *__restrict__ vid, TsdfOut O)
{
    __shared__ float halo[HALO_N];
    BrickVoxel const p = sparse_stage(tsdf, table, list, G, B, halo);
    TsdfGrid const H = halo_grid();
    SPARSE_LOCAL;
    int quads;
    bool active;
    float f[8];
    uint32_t const mine = tsdf_classify<false, true>(halo, H, true, li, lj, lk, f, &active, &quads);
    uint32_t total;
    uint32_t const before = tsdf_block_scan(mine, &total);
    if ((quads & 7) == 0)
        return;
    size_t quad = (size_t)(counts[blockIdx.x] >> 32) + (before >> 16);
    bool const inside = (quads & 8) != 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (!(quads >> a & 1))
            continue;
        uint32_t v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            int cell[3];
            tsdf_quad_cell(a, q, p.i, p.j, p.k, cell);
            // the four cells of a quad are active: in the grid, brick allocated
            size_t at;
            v[q] = 0;
            if (cell[0] >= 0 && cell[1] >= 0 && cell[2] >= 0
                && sparse_at(B, table, cell[0], cell[1], cell[2], &at))
                v[q] = vid[at];
        }
        tsdf_quad_faces(v, inside, O.faces + 6 * quad);
        ++quad;
    }
}

} // namespace smvs_hip

using namespace smvs_hip;
using namespace smvs_hip::tsdf_host;

TsdfBricks
smvs_hip::tsdf_host::brick_grid(TsdfGrid const &G, size_t *n_bricks)
{
    TsdfBricks B;
    B.bx = (G.nx + TSDF_BX - 1) / TSDF_BX;
    B.by = (G.ny + TSDF_BY - 1) / TSDF_BY;
    B.bz = (G.nz + TSDF_BZ - 1) / TSDF_BZ;
    *n_bricks = (size_t)B.bx * B.by * B.bz;
    B.n = (unsigned)*n_bricks;      // the entries refuse more than 2^28
    return B;
}

void
smvs_hip::tsdf_host::BrickWork::carve(const smvs_point_view *views, int n_views, size_t n_bricks,
    bool with_cull, Carver &carve)
{
    cull = with_cull;
    blocks = (unsigned)((n_bricks + 255) / 256);
    size_t const scan_tiles = ((size_t)blocks + SCAN_TILE - 1) / SCAN_TILE;
    seed_at = carve(n_bricks);
    state_at = carve(n_bricks);
    table_at = carve(4 * n_bricks);
    counts_at = carve(8 * (size_t)blocks);
    tiles_at = carve(8 * (scan_tiles + 1));
    if (cull) {
        carve_pyramids(views, n_views, carve, pyr);
        cand_at = carve(n_bricks);
    }
}

void
smvs_hip::tsdf_host::BrickWork::place(char *slab)
{
    seed = reinterpret_cast<uint8_t *>(slab + seed_at);
    state = reinterpret_cast<uint8_t *>(slab + state_at);
    table = reinterpret_cast<int32_t *>(slab + table_at);
    counts = reinterpret_cast<unsigned long long *>(slab + counts_at);
    tiles = reinterpret_cast<unsigned long long *>(slab + tiles_at);
    cand = cull ? reinterpret_cast<uint8_t *>(slab + cand_at) : nullptr;
}

int
smvs_hip::tsdf_host::launch_seeds(Workspace &ws, char *slab, ViewSlab const &s, int n_views,
    TsdfGrid const &G, TsdfBricks const &B, BrickWork &w, uint8_t *brick_candidate,
    size_t *n_tested)
{
    hipStream_t const stream = ws.stream;
    size_t const n_bricks = B.n;
    int rc;
    *n_tested = n_bricks;
    if (w.cull) {
        // the candidates (section 9.10), their list in the table's place, and
        // the exact test on the list alone; the counts are the dilation's, not
        // yet in use
        if ((rc = launch_pyramids(ws, slab, s, n_views, w.pyr)))
            return rc;
        launch_cull(stream, s, w.pyr, G, B, w.cand, w.counts);
        SMVS_HIP_CHECK(hipGetLastError());
        if ((rc = exclusive_scan(stream, w.counts, w.blocks, w.tiles)))
            return rc;
        unsigned long long total = 0;
        if ((rc = ws.download(&total, scan_total(w.tiles, w.blocks), sizeof(total))))
            return rc;
        *n_tested = (size_t)total;
        if (brick_candidate != nullptr && (rc = ws.download(brick_candidate, w.cand, n_bricks)))
            return rc;
        SMVS_HIP_CHECK(hipMemsetAsync(w.seed, 0, n_bricks, stream));
        uint32_t *const cand_list = reinterpret_cast<uint32_t *>(w.table);
        launch_candidate_list(stream, w.cand, B, w.counts, cand_list);
        launch_seed_list(stream, s, G, B, cand_list, *n_tested, w.seed);
    } else {
        if (brick_candidate != nullptr)
            std::memset(brick_candidate, 1, n_bricks);
        // (a launch's x extent in threads is 32 bits: the bricks go over x and y)
        unsigned const seed_x = n_bricks < SEED_GRID_X ? (unsigned)n_bricks : SEED_GRID_X;
        unsigned const seed_y = (unsigned)((n_bricks + SEED_GRID_X - 1) / SEED_GRID_X);
        hipLaunchKernelGGL(tsdf_sparse_seed_kernel, dim3(seed_x, seed_y), dim3(256), 0, stream,
            s.d_table, G, B, w.seed);
    }
    return SMVS_OK;
}

void
smvs_hip::tsdf_host::launch_dilate(hipStream_t stream, const uint8_t *seed, TsdfBricks const &B,
    uint8_t *state, unsigned long long *counts)
{
    hipLaunchKernelGGL(tsdf_sparse_dilate_kernel, dim3((B.n + 255u) / 256u), dim3(256), 0, stream,
        seed, B, state, counts);
}

void
smvs_hip::tsdf_host::launch_table(hipStream_t stream, const uint8_t *state, TsdfBricks const &B,
    const unsigned long long *counts, int32_t *table, uint32_t *list)
{
    hipLaunchKernelGGL(tsdf_sparse_table_kernel, dim3((B.n + 255u) / 256u), dim3(256), 0, stream,
        state, B, counts, table, list);
}

int
smvs_hip::tsdf_host::extract_sparse_surface(Workspace &ws, const char *who, TsdfGrid const &G,
    TsdfBricks const &B, size_t n_alloc, const float *d_tsdf, const uint32_t *d_weight,
    const uint4 *d_colour, const int32_t *d_table, const uint32_t *d_list, float *tsdf,
    uint32_t *weight, smvs_points **handle)
{
    hipStream_t const stream = ws.stream;
    int rc;
    // (no allocated brick or no vertex: no further slab, no launches, an empty handle)
    TsdfOut O = {};
    long long *d_cells = nullptr;
    size_t n_vert = 0, n_face = 0;
    size_t const n_state = n_alloc * 256;
    size_t const n_vox = (size_t)G.nx * G.ny * G.nz;
    if (n_alloc > 0) {
        size_t const scan_tiles = (n_alloc + SCAN_TILE - 1) / SCAN_TILE;
        Carver wc;
        size_t const vid_at = wc(4 * n_state), counts_at = wc(8 * n_alloc),
            tiles_at = wc(8 * (scan_tiles + 1));
        char *work = nullptr;
        if ((rc = ws.ensure(3, wc.total, &work)) != SMVS_OK)
            return rc;
        uint32_t *d_vid = reinterpret_cast<uint32_t *>(work + vid_at);
        unsigned long long *d_counts = reinterpret_cast<unsigned long long *>(work + counts_at);
        unsigned long long *d_tiles = reinterpret_cast<unsigned long long *>(work + tiles_at);
        unsigned const slots = (unsigned)n_alloc;
        hipLaunchKernelGGL(tsdf_sparse_classify_kernel, dim3(slots), dim3(256), 0, stream,
            d_tsdf, d_table, d_list, G, B, d_counts);
        if (hipGetLastError() != hipSuccess) {
            set_error("%s: integration launch failed", who);
            return SMVS_ERR_HIP;
        }
        if ((rc = exclusive_scan(stream, d_counts, n_alloc, d_tiles)))
            return rc;
        unsigned long long sums = 0;
        if ((rc = ws.download(&sums, scan_total(d_tiles, n_alloc), sizeof(sums))))
            return rc;
        n_vert = (size_t)(sums & 0xffffffffull);
        n_face = 2 * (size_t)(sums >> 32);
        if (n_vert > 0) {
            Carver oc;
            size_t const xyz_at = oc(12 * n_vert), nrm_at = oc(12 * n_vert),
                conf_at = oc(4 * n_vert), rgb_at = oc(3 * n_vert), faces_at = oc(12 * n_face),
                cells_at = oc(8 * n_vert);
            char *outs = nullptr;
            if ((rc = ws.ensure(1, oc.total, &outs)) != SMVS_OK)
                return rc;
            O.xyz = reinterpret_cast<float *>(outs + xyz_at);
            O.nrm = reinterpret_cast<float *>(outs + nrm_at);
            O.conf = reinterpret_cast<float *>(outs + conf_at);
            O.rgb = reinterpret_cast<uint8_t *>(outs + rgb_at);
            O.faces = reinterpret_cast<uint32_t *>(outs + faces_at);
            d_cells = reinterpret_cast<long long *>(outs + cells_at);
            hipLaunchKernelGGL(tsdf_sparse_vertex_kernel, dim3(slots), dim3(256), 0, stream,
                d_tsdf, d_weight, d_colour, d_table, d_list, G, B, d_counts, d_vid, O, d_cells);
            hipLaunchKernelGGL(tsdf_sparse_face_kernel, dim3(slots), dim3(256), 0, stream,
                d_tsdf, d_table, d_list, G, B, d_counts, d_vid, O);
            if (hipGetLastError() != hipSuccess) {
                set_error("%s: extraction launch failed", who);
                return SMVS_ERR_HIP;
            }
        }
    }
    smvs_points *h = nullptr;
    if ((rc = fill_points(ws, true, true, n_vert, n_face,
            VertexAttrs{ O.xyz, O.nrm, O.rgb, O.conf, nullptr }, O.faces, d_cells, &h)))
        return rc;
    auto fail = [&](int code) {
        delete h;
        return code;
    };
    std::vector<uint32_t> host_list;
    std::vector<float> host_f;
    std::vector<uint32_t> host_w;
    if (n_alloc > 0 && (tsdf != nullptr || weight != nullptr)) {
        host_list.resize(n_alloc);
        if ((rc = ws.download(host_list.data(), d_list, 4 * n_alloc)))
            return fail(rc);
        if (tsdf != nullptr) {
            host_f.resize(n_state);
            if ((rc = ws.download(host_f.data(), d_tsdf, 4 * n_state)))
                return fail(rc);
        }
        if (weight != nullptr) {
            host_w.resize(n_state);
            if ((rc = ws.download(host_w.data(), d_weight, 4 * n_state)))
                return fail(rc);
        }
    }
    // the whole grid from the slot-major state: NaN / 0 where not allocated
    if (tsdf != nullptr)
        for (size_t p = 0; p < n_vox; ++p)
            tsdf[p] = std::nanf("");
    if (weight != nullptr)
        std::memset(weight, 0, 4 * n_vox);
    for (size_t slot = 0; slot < host_list.size(); ++slot) {
        unsigned const brick = host_list[slot];
        int const i0 = (int)(brick % B.bx) * TSDF_BX, j0 = (int)(brick / B.bx % B.by) * TSDF_BY,
            k0 = (int)(brick / B.bx / B.by) * TSDF_BZ;
        for (int l = 0; l < 256; ++l) {
            int const i = i0 + (l & 7), j = j0 + (l >> 3 & 7), k = k0 + (l >> 6);
            if (i >= G.nx || j >= G.ny || k >= G.nz)
                continue;
            size_t const at = ((size_t)k * G.ny + j) * G.nx + i;
            if (tsdf != nullptr)
                tsdf[at] = host_f[slot * 256 + l];
            if (weight != nullptr)
                weight[at] = host_w[slot * 256 + l];
        }
    }
    *handle = h;
    return SMVS_OK;
}

extern "C" int
smvs_tsdf_fuse_sparse(int device, const smvs_point_view *views, int n_views,
    const smvs_tsdf_options *options, const smvs_tsdf_sparse_options *sparse,
    uint8_t *brick_state, float *tsdf, uint32_t *weight, smvs_tsdf_sparse_stats *stats,
    smvs_points **handle, int64_t *n_vertices, int64_t *n_faces)
{
    smvs_tsdf_sparse_opts o;
    o.max_bricks = sparse != nullptr ? sparse->max_bricks : 0;
    o.cull = 0;
    smvs_tsdf_sparse_opts_stats st = {};
    int const rc = smvs_tsdf_fuse_sparse_opts(device, views, n_views, options, &o, brick_state,
        nullptr, tsdf, weight, stats != nullptr ? &st : nullptr, handle, n_vertices, n_faces);
    // (the stats are filled from the seed and dilation passes on, with SMVS_ERR_NOMEM too)
    if (stats != nullptr && st.bricks != 0) {
        stats->bricks = st.bricks;
        stats->seed_bricks = st.seed_bricks;
        stats->allocated_bricks = st.allocated_bricks;
        stats->state_bytes = st.state_bytes;
    }
    return rc;
}

extern "C" int
smvs_tsdf_fuse_sparse_opts(int device, const smvs_point_view *views, int n_views,
    const smvs_tsdf_options *options, const smvs_tsdf_sparse_opts *sparse,
    uint8_t *brick_state, uint8_t *brick_candidate, float *tsdf, uint32_t *weight,
    smvs_tsdf_sparse_opts_stats *stats, smvs_points **handle, int64_t *n_vertices,
    int64_t *n_faces)
{
    SMVS_REQUIRE(handle != nullptr, "no handle pointer");
    *handle = nullptr;
    SMVS_REQUIRE(options != nullptr, "no options");
    smvs_tsdf_options const &opt = *options;
    int rc;
    if ((rc = check_views(views, n_views, opt.cut_surfaces, true)))
        return rc;
    TsdfGrid G;
    if ((rc = check_grid("smvs_tsdf_fuse_sparse", opt, n_views, 4096, G)))
        return rc;
    size_t n_bricks;
    TsdfBricks const B = brick_grid(G, &n_bricks);
    SMVS_REQUIRE(n_bricks <= MAX_BRICKS_GRID, "the brick grid has more than 2^28 bricks");
    size_t const n_vox = (size_t)G.nx * G.ny * G.nz;
    SMVS_REQUIRE((tsdf == nullptr && weight == nullptr) || n_vox <= TSDF_MAX_VOXELS,
        "tsdf / weight are given only for grids of at most 2^27 voxels");
    int64_t max_bricks = sparse != nullptr ? sparse->max_bricks : 0;
    if (max_bricks <= 0)
        max_bricks = DEFAULT_MAX_BRICKS;
    SMVS_REQUIRE(max_bricks <= MAX_MAX_BRICKS, "max_bricks must be at most 2^23");
    bool const cull = sparse != nullptr && sparse->cull != 0;

    WorkspaceLease lease(device);
    if (lease.w == nullptr)
        return SMVS_ERR_HIP;
    Workspace &ws = *lease.w;
    ViewStage stage;
    BrickWork w;
    if ((rc = stage(ws, views, n_views, opt.cut_surfaces != 0, true,
            [&](Carver &carve) { w.carve(views, n_views, n_bricks, cull, carve); })))
        return rc;
    hipStream_t const stream = ws.stream;
    ViewSlab const &s = stage.s;
    w.place(stage.slab);

    size_t n_tested = n_bricks;
    if ((rc = launch_seeds(ws, stage.slab, s, n_views, G, B, w, brick_candidate, &n_tested)))
        return rc;
    hipLaunchKernelGGL(tsdf_sparse_dilate_kernel, dim3(w.blocks), dim3(256), 0, stream, w.seed, B,
        w.state, w.counts);
    SMVS_HIP_CHECK(hipGetLastError());
    if ((rc = exclusive_scan(stream, w.counts, w.blocks, w.tiles)))
        return rc;
    unsigned long long sums = 0;
    if ((rc = ws.download(&sums, scan_total(w.tiles, w.blocks), sizeof(sums))))
        return rc;
    size_t const n_alloc = (size_t)(sums & 0xffffffffull);
    if (stats != nullptr) {
        stats->bricks = (int64_t)n_bricks;
        stats->seed_bricks = (int64_t)(sums >> 32);
        stats->allocated_bricks = (int64_t)n_alloc;
        stats->state_bytes = (int64_t)n_alloc * ONE_SHOT_STATE_BYTES_PER_BRICK;
        stats->tested_bricks = (int64_t)n_tested;
    }
    if (brick_state != nullptr && (rc = ws.download(brick_state, w.state, n_bricks)))
        return rc;
    if ((int64_t)n_alloc > max_bricks) {
        set_error("smvs_tsdf_fuse_sparse: the surface needs %lld bricks (%lld bytes of state), "
            "max_bricks is %lld", (long long)n_alloc,
            (long long)n_alloc * (long long)ONE_SHOT_STATE_BYTES_PER_BRICK,
            (long long)max_bricks);
        return SMVS_ERR_NOMEM;
    }

    // (no allocated brick: no further slab, no launches, an empty handle)
    size_t const n_state = n_alloc * 256;
    uint32_t *d_list = nullptr;
    float *d_tsdf = nullptr;
    uint32_t *d_weight = nullptr;
    uint4 *d_colour = nullptr;
    if (n_alloc > 0) {
        Carver vc;
        size_t const list_at = vc(4 * n_alloc), f_at = vc(4 * n_state), w_at = vc(4 * n_state),
            colour_at = vc(16 * n_state);
        char *vol = nullptr;
        if ((rc = ws.ensure(2, vc.total, &vol)) != SMVS_OK)
            return rc;
        d_list = reinterpret_cast<uint32_t *>(vol + list_at);
        d_tsdf = reinterpret_cast<float *>(vol + f_at);
        d_weight = reinterpret_cast<uint32_t *>(vol + w_at);
        d_colour = reinterpret_cast<uint4 *>(vol + colour_at);
        hipLaunchKernelGGL(tsdf_sparse_table_kernel, dim3(w.blocks), dim3(256), 0, stream,
            w.state, B, w.counts, w.table, d_list);
        hipLaunchKernelGGL(tsdf_sparse_integrate_kernel, dim3((unsigned)n_alloc), dim3(256), 0,
            stream, s.d_table, stage.d_images, G, B, d_list, d_tsdf, d_weight, d_colour);
    }
    // classify, scan, vertices, faces, fill: the half smvs_tsdf_sparse_volume_extract shares
    smvs_points *h = nullptr;
    if ((rc = extract_sparse_surface(ws, "smvs_tsdf_fuse_sparse", G, B, n_alloc, d_tsdf, d_weight,
            d_colour, w.table, d_list, tsdf, weight, &h)))
        return rc;
    return publish(h, handle, n_vertices, n_faces);
}

extern "C" int
smvs_tsdf_vertex_cells(const smvs_points *handle, int64_t *cell)
{
    SMVS_REQUIRE(handle != nullptr && cell != nullptr, "no handle or no output");
    SMVS_REQUIRE(handle->sparse, "not a handle of smvs_tsdf_fuse_sparse");
    if (!handle->cells.empty())
        std::memcpy(cell, handle->cells.data(), sizeof(int64_t) * handle->cells.size());
    return SMVS_OK;
}
