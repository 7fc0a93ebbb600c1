// Volumetric fusion of the depth maps into one surface mesh on gfx950
// (not in the reference, opt-in).  The normative
// definition is the comment of smvs_tsdf_fuse in include/smvs_hip.h, restated
// in numpy by tests/tsdf_ref.py; every step below names the paragraph it
// implements.
//
// The views are prepared exactly as the mesh export prepares them (the view
// stage of mesh_cut.hip: carve_views / upload_and_prepare), then
//   depth      per pixel: D = depth_z where the cut map is non-zero, else 0
//   integrate  one lane per voxel walks the views in list order with the
//              voxel's sums in registers; the volume is written once
//   classify   per block of 256 grid points: active cells | quads << 32
//   scan       export_common.hip's exclusive_scan over the blocks
//   vertices   one surface-nets vertex per active cell, with its attributes,
//              and the cell -> vertex id map
//   faces      two triangles per quad through that map
//   fill       export_common.hip's fill_points
// Arithmetic: float, FMA contraction off, term by term as mesh.hip writes it.
// No atomics: every order is an index order (vertex ids and face positions
// come from the scan and a scan inside each block).
// The per-element device functions live in tsdf_shared.h, which
// tsdf_sparse.hip (the brick-sparse volume, section 9.9) uses as well; the
// extraction half of the entry is tsdf_host::extract_surface, which
// tsdf_volume.hip (the persistent volume, section 9.13) runs on its own sums.
#include "common.h"
#include "mesh_shared.h"
#include "tsdf_shared.h"

#include <cmath>
#include <vector>

namespace smvs_hip {

__device__ __forceinline__ bool
tsdf_pixel(const MeshViewDev *views, int &v, int &x, int &y, size_t &p)
{
    v = blockIdx.y;
    MeshViewDev const &V = views[v];
    size_t const local = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (local >= (size_t)V.w * V.h)
        return false;
    x = (int)(local % V.w);
    y = (int)(local / V.w);
    p = local;
    return true;
}

// Inputs: D(p) = depth_z[p] where cut[p] != 0, else 0 (in place in depth_z,
// which nothing else reads after the cut)
__global__ void __launch_bounds__(256)
tsdf_depth_kernel(const MeshViewDev *__restrict__ views)
{
    int v, x, y;
    size_t p;
    if (!tsdf_pixel(views, v, x, y, p))
        return;
    if (views[v].cut[p] == 0.0f)
        views[v].depth_z[p] = 0.0f;
}

// Field, steps 1-8 and the division after the loop.  A block is a brick of
// 8 x 8 x 4 voxels (tsdf_shared.h).
__global__ void __launch_bounds__(256)
tsdf_integrate_kernel(const MeshViewDev *__restrict__ views,
    const TsdfImageDev *__restrict__ images, TsdfGrid G, float *__restrict__ tsdf,
    uint32_t *__restrict__ weight, uint4 *__restrict__ colour)
{
#pragma clang fp contract(off)
    int const bricks_x = (G.nx + TSDF_BX - 1) / TSDF_BX;
    int const bricks_y = (G.ny + TSDF_BY - 1) / TSDF_BY;
    int const brick = blockIdx.x;
    int const i = (brick % bricks_x) * TSDF_BX + (threadIdx.x & 7);
    int const j = (brick / bricks_x % bricks_y) * TSDF_BY + (threadIdx.x >> 3 & 7);
    int const k = (brick / bricks_x / bricks_y) * TSDF_BZ + (threadIdx.x >> 6);
    if (i >= G.nx || j >= G.ny || k >= G.nz)
        return;
    float const c[3] = { tsdf_centre(G, 0, i), tsdf_centre(G, 1, j), tsdf_centre(G, 2, k) };
    float S = 0.0f;
    uint32_t W = 0, R = 0, Gr = 0, B = 0, C = 0;
    for (int v = 0; v < G.n_views; ++v) {
        MeshViewDev const &V = views[v];
        TSDF_STEPS_1_TO_6(V, c, G.trunc, continue);
        S += fminf(1.0f, sdf / G.trunc);
        W += 1;
        if (sdf <= G.trunc) {
            int const ch = images[v].channels;
            const uint8_t *px = images[v].image + pj * ch;
            uint32_t const g = px[0];
            R += g;
            Gr += ch >= 3 ? px[1] : g;
            B += ch >= 3 ? px[2] : g;
            C += 1;
        }
    }
    size_t const at = ((size_t)k * G.ny + j) * G.nx + i;
    tsdf[at] = W >= G.min_weight ? S / (float)W : __builtin_nanf("");
    weight[at] = W;
    colour[at] = make_uint4(R, Gr, B, C);
}

// ----------------------------------------------------------------- extraction
// Cells and grid points share the points' linear index (x fastest): cell
// (i, j, k) is the one whose corner 0 is point (i, j, k).

__device__ __forceinline__ bool
tsdf_point(TsdfGrid const &G, size_t &lin, int &i, int &j, int &k)
{
    lin = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (lin >= (size_t)G.nx * G.ny * G.nz)
        return false;
    i = (int)(lin % G.nx);
    j = (int)(lin / G.nx % G.ny);
    k = (int)(lin / G.nx / G.ny);
    return true;
}

__global__ void __launch_bounds__(256)
tsdf_classify_kernel(const float *__restrict__ tsdf, TsdfGrid G,
    unsigned long long *__restrict__ counts)
{
    size_t lin;
    int i = 0, j = 0, k = 0, quads;
    bool active;
    float f[8];
    bool const valid = tsdf_point(G, lin, i, j, k);
    uint32_t const mine = tsdf_classify<true, true>(tsdf, G, valid, i, j, k, f, &active, &quads);
    uint32_t total;
    (void)tsdf_block_scan(mine, &total);
    if (threadIdx.x == 0)
        counts[blockIdx.x] = (unsigned long long)(total & 0xffffu)
            | (unsigned long long)(total >> 16) << 32;
}

// Vertices: position, normal, colour, confidence of every active cell, at the
// cell's rank; vid[cell] = that rank
__global__ void __launch_bounds__(256)
tsdf_vertex_kernel(const float *__restrict__ tsdf, const uint32_t *__restrict__ weight,
    const uint4 *__restrict__ colour, TsdfGrid G,
    const unsigned long long *__restrict__ counts, uint32_t *__restrict__ vid, TsdfOut O)
{
#pragma clang fp contract(off)
    size_t lin;
    int i = 0, j = 0, k = 0, quads;
    bool active;
    float f[8];
    bool const valid = tsdf_point(G, lin, i, j, k);
    uint32_t const mine = tsdf_classify<true, false>(tsdf, G, valid, i, j, k, f, &active, &quads);
    uint32_t total;
    uint32_t const before = tsdf_block_scan(mine, &total);
    if (!active)
        return;
    size_t const id = (size_t)(uint32_t)counts[blockIdx.x] + (before & 0xffffu);
    vid[lin] = (uint32_t)id;
    int const cell[3] = { i, j, k };
    TSDF_VERTEX_GEOMETRY(G, cell, f, id, O);
    uint32_t Rs = 0, Gs = 0, Bs = 0, Cs = 0, Ws = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        size_t const at = tsdf_index(G, i + (c & 1), j + (c >> 1 & 1), k + (c >> 2));
        uint4 const col = colour[at];
        Rs += col.x;
        Gs += col.y;
        Bs += col.z;
        Cs += col.w;
        Ws += weight[at];
    }
    TSDF_VERTEX_ATTRIBUTES(G, Rs, Gs, Bs, Cs, Ws, id, O);
}

// Faces: the quads of every grid point in linear order, axes 0, 1, 2 in turn,
// two triangles each, counter-clockwise seen from outside
__global__ void __launch_bounds__(256)
tsdf_face_kernel(const float *__restrict__ tsdf, TsdfGrid G,
    const unsigned long long *__restrict__ counts, const uint32_t *__restrict__ vid,
    TsdfOut O)
{
    size_t lin;
    int i = 0, j = 0, k = 0, quads;
    bool active;
    float f[8];
    bool const valid = tsdf_point(G, lin, i, j, k);
    uint32_t const mine = tsdf_classify<false, true>(tsdf, G, valid, i, j, k, f, &active, &quads);
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
            tsdf_quad_cell(a, q, i, j, k, cell);
            v[q] = vid[tsdf_index(G, cell[0], cell[1], cell[2])];
        }
        tsdf_quad_faces(v, inside, O.faces + 6 * quad);
        ++quad;
    }
}

// --------------------------------------------------------------------- bounds
// min and max of world_point over the valid pixels of the (cut) maps: per
// block, then one block over the blocks' results.  Exact, so no order matters.
__device__ __forceinline__ void
tsdf_block_minmax(float *lo, float *hi, float *out)
{
    __shared__ float part[4][6];
    int const lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lo[r] = fminf(lo[r], __shfl_xor(lo[r], o, 64));
            hi[r] = fmaxf(hi[r], __shfl_xor(hi[r], o, 64));
        }
    if (lane == 0)
        for (int r = 0; r < 3; ++r) {
            part[wave][r] = lo[r];
            part[wave][3 + r] = hi[r];
        }
    __syncthreads();
    if (threadIdx.x < 6) {
        float v = part[0][threadIdx.x];
        for (int w = 1; w < 4; ++w)
            v = threadIdx.x < 3 ? fminf(v, part[w][threadIdx.x])
                                : fmaxf(v, part[w][threadIdx.x]);
        out[threadIdx.x] = v;
    }
}

__global__ void __launch_bounds__(256)
tsdf_bounds_kernel(const MeshViewDev *__restrict__ views, float *__restrict__ partial)
{
    float const inf = __builtin_huge_valf();
    float lo[3] = { inf, inf, inf }, hi[3] = { -inf, -inf, -inf };
    int v, x, y;
    size_t p;
    if (tsdf_pixel(views, v, x, y, p)) {
        float const d = views[v].cut[p];
        if (d != 0.0f) {
            float pos[3];
            world_point(views[v], x, y, d, pos);
            for (int r = 0; r < 3; ++r)
                lo[r] = hi[r] = pos[r];
        }
    }
    tsdf_block_minmax(lo, hi, partial + 6 * ((size_t)blockIdx.y * gridDim.x + blockIdx.x));
}

__global__ void __launch_bounds__(256)
tsdf_bounds_final_kernel(const float *__restrict__ partial, size_t n, float *__restrict__ out)
{
    float const inf = __builtin_huge_valf();
    float lo[3] = { inf, inf, inf }, hi[3] = { -inf, -inf, -inf };
    for (size_t b = threadIdx.x; b < n; b += 256)
        for (int r = 0; r < 3; ++r) {
            lo[r] = fminf(lo[r], partial[6 * b + r]);
            hi[r] = fmaxf(hi[r], partial[6 * b + 3 + r]);
        }
    tsdf_block_minmax(lo, hi, out);
}

// the host pieces tsdf_sparse.hip uses as well (declared in tsdf_shared.h)
namespace tsdf_host {

// argument checks shared by the entries (before any device call)
int
check_views(const smvs_point_view *views, int n_views, int cut, bool want_images)
{
    SMVS_REQUIRE(views != nullptr && n_views >= 1, "no views");
    SMVS_REQUIRE(n_views <= 4096, "too many views");
    size_t total_pix = 0;
    for (int i = 0; i < n_views; ++i) {
        smvs_point_view const &in = views[i];
        SMVS_REQUIRE(in.width > 0 && in.height > 0 && in.depth != nullptr
            && in.flen > 0.0f, "bad view");
        SMVS_REQUIRE(!want_images || (in.image != nullptr && in.channels >= 1
            && in.channels <= 4), "bad view image");
        SMVS_REQUIRE(!(cut && in.normals == nullptr),
            "the cut needs the normal maps");
        total_pix += (size_t)in.width * in.height;
    }
    SMVS_REQUIRE(total_pix < ((size_t)1 << 31), "too many pixels");
    return SMVS_OK;
}

int
upload_image_table(Workspace &ws, char *slab, size_t at, const smvs_point_view *views,
    ViewSlab const &s, TsdfImageDev **d_images)
{
    std::vector<TsdfImageDev> images(s.images.size());
    for (size_t i = 0; i < images.size(); ++i) {
        images[i].image = s.images[i];
        images[i].channels = views[i].channels;
    }
    *d_images = reinterpret_cast<TsdfImageDev *>(slab + at);
    return ws.upload(*d_images, images.data(), sizeof(TsdfImageDev) * images.size());
}

int
check_grid(const char *who, const smvs_tsdf_options &opt, int n_views, int max_dim,
    TsdfGrid &G)
{
    auto refuse = [&](const char *msg) {
        set_error("%s: %s", who, msg);
        return SMVS_ERR_INVALID;
    };
    if (!(std::isfinite(opt.voxel_size) && opt.voxel_size > 0.0f))
        return refuse("voxel_size must be positive and finite");
    if (!std::isfinite(opt.trunc))
        return refuse("trunc must be finite");
    for (int r = 0; r < 3; ++r) {
        if (!(opt.dims[r] >= 2 && opt.dims[r] <= max_dim))
            return refuse(max_dim == 1024 ? "dims must be 2 .. 1024" : "dims must be 2 .. 4096");
        if (!std::isfinite(opt.origin[r]))
            return refuse("origin must be finite");
    }
    G.nx = opt.dims[0];
    G.ny = opt.dims[1];
    G.nz = opt.dims[2];
    for (int r = 0; r < 3; ++r)
        G.origin[r] = opt.origin[r];
    G.voxel_size = opt.voxel_size;
    G.trunc = opt.trunc > 0.0f ? opt.trunc : 3.0f * opt.voxel_size;
    G.min_weight = opt.min_weight > 0 ? (uint32_t)opt.min_weight : 1u;
    G.n_views = n_views;
    return SMVS_OK;
}

void
launch_depth(hipStream_t stream, ViewSlab const &s, int n_views)
{
    hipLaunchKernelGGL(tsdf_depth_kernel, dim3((unsigned)((s.max_pix + 255) / 256),
        (unsigned)n_views), dim3(256), 0, stream, s.d_table);
}

void
carve_extract(size_t n_vox, Carver &carve, ExtractPieces &at)
{
    at.point_blocks = (unsigned)((n_vox + 255) / 256);
    size_t const scan_tiles = ((size_t)at.point_blocks + SCAN_TILE - 1) / SCAN_TILE;
    at.vid = carve(4 * n_vox);
    at.counts = carve(8 * (size_t)at.point_blocks);
    at.tiles = carve(8 * (scan_tiles + 1));
}

int
extract_surface(Workspace &ws, const char *who, TsdfGrid const &G, char *slab,
    ExtractPieces const &at, const float *d_tsdf, const uint32_t *d_weight,
    const uint4 *d_colour, smvs_points **handle)
{
    hipStream_t const stream = ws.stream;
    unsigned const point_blocks = at.point_blocks;
    uint32_t *d_vid = reinterpret_cast<uint32_t *>(slab + at.vid);
    unsigned long long *d_counts = reinterpret_cast<unsigned long long *>(slab + at.counts);
    unsigned long long *d_tiles = reinterpret_cast<unsigned long long *>(slab + at.tiles);
    int rc;
    hipLaunchKernelGGL(tsdf_classify_kernel, dim3(point_blocks), dim3(256), 0, stream, d_tsdf,
        G, d_counts);
    SMVS_HIP_CHECK(hipGetLastError());
    if ((rc = exclusive_scan(stream, d_counts, point_blocks, d_tiles)))
        return rc;
    unsigned long long sums = 0;
    if ((rc = ws.download(&sums, scan_total(d_tiles, point_blocks), sizeof(sums))))
        return rc;
    size_t const n_vert = (size_t)(sums & 0xffffffffull);
    size_t const n_face = 2 * (size_t)(sums >> 32);

    // (no vertices: no second slab, no launches, an empty handle)
    TsdfOut O = {};
    if (n_vert > 0) {
        Carver oc;
        size_t const xyz_at = oc(12 * n_vert), nrm_at = oc(12 * n_vert), conf_at = oc(4 * n_vert),
            rgb_at = oc(3 * n_vert), faces_at = oc(12 * n_face);
        char *outs = nullptr;
        if ((rc = ws.ensure(1, oc.total, &outs)) != SMVS_OK)
            return rc;
        O.xyz = reinterpret_cast<float *>(outs + xyz_at);
        O.nrm = reinterpret_cast<float *>(outs + nrm_at);
        O.conf = reinterpret_cast<float *>(outs + conf_at);
        O.rgb = reinterpret_cast<uint8_t *>(outs + rgb_at);
        O.faces = reinterpret_cast<uint32_t *>(outs + faces_at);
        hipLaunchKernelGGL(tsdf_vertex_kernel, dim3(point_blocks), dim3(256), 0, stream,
            d_tsdf, d_weight, d_colour, G, d_counts, d_vid, O);
        hipLaunchKernelGGL(tsdf_face_kernel, dim3(point_blocks), dim3(256), 0, stream, d_tsdf,
            G, d_counts, d_vid, O);
        if (hipGetLastError() != hipSuccess) {
            set_error("%s: extraction launch failed", who);
            return SMVS_ERR_HIP;
        }
    }
    return fill_points(ws, true, false, n_vert, n_face,
        VertexAttrs{ O.xyz, O.nrm, O.rgb, O.conf, nullptr }, O.faces, nullptr, handle);
}

} // namespace tsdf_host

} // namespace smvs_hip

using namespace smvs_hip;
using namespace smvs_hip::tsdf_host;

extern "C" int
smvs_tsdf_bounds(int device, const smvs_point_view *views, int n_views, int cut_surfaces,
    float *lo, float *hi)
{
    SMVS_REQUIRE(lo != nullptr && hi != nullptr, "no output");
    int rc;
    if ((rc = check_views(views, n_views, cut_surfaces, false)))
        return rc;
    WorkspaceLease lease(device);
    if (lease.w == nullptr)
        return SMVS_ERR_HIP;
    Workspace &ws = *lease.w;
    Carver carve;
    ViewSlab s;
    carve_views(views, n_views, false, carve, s);
    unsigned const blocks = (unsigned)((s.max_pix + 255) / 256);
    size_t const n_partial = (size_t)blocks * n_views;
    size_t const partial_at = carve(sizeof(float) * 6 * n_partial);
    size_t const result_at = carve(sizeof(float) * 6);
    char *slab = nullptr;
    if ((rc = ws.ensure(0, carve.total, &slab)) != SMVS_OK)
        return rc;
    if ((rc = upload_and_prepare(ws, slab, views, n_views, cut_surfaces != 0, false, s)))
        return rc;
    float *partial = reinterpret_cast<float *>(slab + partial_at);
    float *result = reinterpret_cast<float *>(slab + result_at);
    hipLaunchKernelGGL(tsdf_bounds_kernel, dim3(blocks, (unsigned)n_views), dim3(256), 0,
        ws.stream, s.d_table, partial);
    hipLaunchKernelGGL(tsdf_bounds_final_kernel, dim3(1), dim3(256), 0, ws.stream, partial,
        n_partial, result);
    SMVS_HIP_CHECK(hipGetLastError());
    float out[6];
    if ((rc = ws.download(out, result, sizeof(out))))
        return rc;
    for (int r = 0; r < 3; ++r) {
        lo[r] = out[r];
        hi[r] = out[3 + r];
    }
    return SMVS_OK;
}

extern "C" int
smvs_tsdf_fuse(int device, const smvs_point_view *views, int n_views,
    const smvs_tsdf_options *options, float *tsdf, uint32_t *weight, smvs_points **handle,
    int64_t *n_vertices, int64_t *n_faces)
{
    SMVS_REQUIRE(handle != nullptr, "no handle pointer");
    *handle = nullptr;
    SMVS_REQUIRE(options != nullptr, "no options");
    smvs_tsdf_options const &opt = *options;
    int rc;
    if ((rc = check_views(views, n_views, opt.cut_surfaces, true)))
        return rc;
    TsdfGrid G;
    if ((rc = check_grid("smvs_tsdf_fuse", opt, n_views, 1024, G)))
        return rc;
    size_t const n_vox = (size_t)G.nx * G.ny * G.nz;
    SMVS_REQUIRE(n_vox <= TSDF_MAX_VOXELS, "the volume has more than 2^27 voxels");

    WorkspaceLease lease(device);
    if (lease.w == nullptr)
        return SMVS_ERR_HIP;
    Workspace &ws = *lease.w;
    ViewStage stage;
    size_t tsdf_at = 0, weight_at = 0, colour_at = 0;
    ExtractPieces extract_at;
    if ((rc = stage(ws, views, n_views, opt.cut_surfaces != 0, true, [&](Carver &carve) {
            tsdf_at = carve(4 * n_vox);
            weight_at = carve(4 * n_vox);
            colour_at = carve(16 * n_vox);
            carve_extract(n_vox, carve, extract_at);
        })))
        return rc;
    char *const slab = stage.slab;
    float *d_tsdf = reinterpret_cast<float *>(slab + tsdf_at);
    uint32_t *d_weight = reinterpret_cast<uint32_t *>(slab + weight_at);
    uint4 *d_colour = reinterpret_cast<uint4 *>(slab + colour_at);

    size_t n_bricks;
    unsigned const bricks = brick_grid(G, &n_bricks).n;
    hipLaunchKernelGGL(tsdf_integrate_kernel, dim3(bricks), dim3(256), 0, ws.stream,
        stage.s.d_table, stage.d_images, G, d_tsdf, d_weight, d_colour);
    smvs_points *h = nullptr;
    if ((rc = extract_surface(ws, "smvs_tsdf_fuse", G, slab, extract_at, d_tsdf, d_weight,
            d_colour, &h)))
        return rc;
    if ((tsdf != nullptr && (rc = ws.download(tsdf, d_tsdf, 4 * n_vox)))
        || (weight != nullptr && (rc = ws.download(weight, d_weight, 4 * n_vox)))) {
        delete h;
        return rc;
    }
    return publish(h, handle, n_vertices, n_faces);
}
