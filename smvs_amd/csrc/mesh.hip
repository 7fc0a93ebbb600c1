// Point and triangle-mesh export on gfx950 (smvs_points_generate,
// smvs_mesh_generate).  The views come out of the shared view stage
// (mesh_cut.hip); the scan, the AABB vertex clip and the result fill are
// export_common.hip's (export_shared.h).
//
// Point export: generate_mesh :217-297 for every view on the device, merged
// in view-list order, and smvsrecon's AABB clip (app/smvsrecon.cc:306-319).
// The MVE pieces (depthmap_triangulate, MeshInfo, depthmap_mesh_confidences,
// save_ply_mesh) follow the [MVE-unverified] table of DESIGN.md section 9.
//
// Per-pixel arrays of all views are concatenated (view v starts at pixel
// off[v]); a 2 x 2 block is indexed by its corner-0 pixel (x, y), so blocks
// and vertices share one index space.  Passes:
//   code   one byte per block: depthmap_triangulate's <= 2 triangles
//   count  new vertices (corners no earlier block uses) | triangles << 32
//   scan   exclusive prefix over all blocks of all views (no atomics): vertex
//          and face ids in MVE's lazy creation order, view after view
//   vid    pixel -> vertex id
//   topo   per pixel: MeshInfo's chained one-ring, vertex class
//   ring   3 relaxations of the distance to the nearest border vertex
//   emit   position, colour, normal, confidence, scale value (and faces)
//   clip   keep flags, scan, order-preserving compaction (AABB only)
// The triangle mesh (smvs_mesh_generate) runs the same
// passes up to emit (without normal and scale value), then
//   normals  recalc_normals as a per-vertex gather over the incident faces
//   clip     as above, plus kept faces per block, their scan and a scatter
//            that renumbers the faces' vertices (AABB only)
// Arithmetic: float, in the reference's operation order, FMA contraction off.
#include "common.h"
#include "export_shared.h"
#include "mesh_shared.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace smvs_hip {

struct PointViewDev {
    int w, h, channels;
    size_t off;             // first pixel of the view in the per-pixel arrays
    const float *dm;        // the triangulated map: cut (ray length) or input
    const uint8_t *image;   // w * h * channels
};

struct PointBufs {
    uint8_t *code;                  // per block
    unsigned long long *scan;       // per block: counts, then their prefix
    unsigned long long *tiles;      // per scan tile (+ the grand total)
    uint32_t *vid;                  // per pixel (used pixels only)
    uint32_t *nbr;                  // per pixel: one-ring, 4-bit directions
    uint8_t *meta;                  // per pixel: count | border << 4 | used << 5
    uint8_t *dist[2];               // per pixel: ring distance (ping-pong)
    float *xyz, *nrm, *conf, *val;  // per vertex (SoA)
    uint8_t *rgb;
    uint32_t *faces;                // per face, 3 vertex ids (or nullptr)
    float dd_factor;
};

// depthmap_triangulate's triangles, corners of the 2 x 2 block:
// 0 = (x, y), 1 = (x + 1, y), 2 = (x, y + 1), 3 = (x + 1, y + 1)
__device__ __forceinline__ int
tri_corner(int t, int k)   // t = 1..4, k = 0..2
{
    // {0,2,1} {0,3,1} {0,2,3} {1,2,3}, two bits per corner
    constexpr unsigned table = (0u | 2u << 2 | 1u << 4)
        | (0u | 3u << 2 | 1u << 4) << 6
        | (0u | 2u << 2 | 3u << 4) << 12
        | (1u | 2u << 2 | 3u << 4) << 18;
    return (table >> (6 * (t - 1) + 2 * k)) & 3;
}

__device__ __forceinline__ int
tri_mask(int t)            // corners of triangle t as bits (t = 0: none)
{
    return (0xEDB70 >> (4 * t)) & 15;   // 0, 0x7, 0xB, 0xD, 0xE
}

__device__ __forceinline__ int
code_mask(int code)
{
    return tri_mask(code & 7) | tri_mask((code >> 3) & 7);
}

// mve::geom::pixel_footprint: invproj[0] * depth / |invproj * (x+.5, y+.5, 1)|
__device__ __forceinline__ float
pixel_footprint(MeshViewDev const &V, int x, int y, float depth)
{
#pragma clang fp contract(off)
    float const px = (float)x + 0.5f, py = (float)y + 0.5f;
    float v[3];
    for (int r = 0; r < 3; ++r) {
        float s = 0.0f;
        s += V.invproj[3 * r] * px;
        s += V.invproj[3 * r + 1] * py;
        s += V.invproj[3 * r + 2] * 1.0f;
        v[r] = s;
    }
    return V.invproj[0] * depth / sqrtf(dot3(v, v));
}

// dm_is_depthdisc: d_max - d_min > footprint(d_min) * dd_factor, the factor
// times MATH_SQRT2 (double) on the diagonals 0-3 and 1-2
__device__ __forceinline__ bool
depth_disc(const float *wd, const float *d, float dd_factor, int i1, int i2)
{
#pragma clang fp contract(off)
    int i_min = i1, i_max = i2;
    if (d[i2] < d[i1]) {
        i_min = i2;
        i_max = i1;
    }
    if (i1 + i2 == 3)
        dd_factor = (float)((double)dd_factor * 1.41421356237309504880);
    return d[i_max] - d[i_min] > wd[i_min] * dd_factor;
}

// the triangles of block (x, y): tri[0] | tri[1] << 3, each 0 (none) or 1..4
__device__ int
block_code(MeshViewDev const &V, const float *dm, int x, int y, float dd_factor)
{
#pragma clang fp contract(off)
    size_t const i = (size_t)y * V.w + x;
    float const d[4] = { dm[i], dm[i + 1], dm[i + V.w], dm[i + V.w + 1] };
    int mask = 0, n = 0;
    for (int j = 0; j < 4; ++j)
        if (d[j] > 0.0f) {
            mask |= 1 << j;
            ++n;
        }
    if (n < 3)
        return 0;
    int tri[2] = { 0, 0 };
    switch (mask) {
    case 7: tri[0] = 1; break;
    case 11: tri[0] = 2; break;
    case 13: tri[0] = 3; break;
    case 14: tri[0] = 4; break;
    default: {
        float const dd1 = fabsf(d[0] - d[3]);
        float const dd2 = fabsf(d[1] - d[2]);
        if (dd1 < dd2) {
            tri[0] = 2;
            tri[1] = 3;
        } else {
            tri[0] = 1;
            tri[1] = 4;
        }
    }
    }
    if (dd_factor > 0.0f) {
        float wd[4];
        for (int j = 0; j < 4; ++j)
            wd[j] = d[j] == 0.0f ? 0.0f
                : pixel_footprint(V, x + (j & 1), y + (j >> 1), d[j]);
        for (int j = 0; j < 2 && tri[j] != 0; ++j) {
            int const a = tri_corner(tri[j], 0), b = tri_corner(tri[j], 1),
                c = tri_corner(tri[j], 2);
            if (depth_disc(wd, d, dd_factor, a, b)
                || depth_disc(wd, d, dd_factor, b, c)
                || depth_disc(wd, d, dd_factor, c, a))
                tri[j] = 0;
        }
    }
    return tri[0] | tri[1] << 3;
}

// Corners of block (x, y) that become vertices here (dm_make_triangle: the
// first triangle in emission order that uses a pixel creates its vertex), in
// creation order as 2-bit corners; -> their number.  Earlier blocks that
// share a corner: (x-1, y-1), (x, y-1), (x+1, y-1), (x-1, y).
__device__ __forceinline__ int
block_new_corners(const uint8_t *code, int w, int x, int y, int c, int *order)
{
    size_t const i = (size_t)y * w + x;
    int earlier = 0;
    if (y > 0) {
        int const up = code_mask(code[i - w]);
        int const up_right = code_mask(code[i - w + 1]);   // x + 1 <= w - 1
        earlier |= (up >> 2 & 1) | (up >> 3 & 1) << 1 | (up_right >> 2 & 1) << 1;
        if (x > 0)
            earlier |= code_mask(code[i - w - 1]) >> 3 & 1;
    }
    if (x > 0) {
        int const left = code_mask(code[i - 1]);
        earlier |= (left >> 1 & 1) | (left >> 3 & 1) << 2;
    }
    int fresh = code_mask(c) & ~earlier;
    int n = 0, packed = 0;
    for (int j = 0; j < 2; ++j) {
        int const t = (c >> (3 * j)) & 7;
        if (t == 0)
            continue;
        for (int k = 0; k < 3; ++k) {
            int const cc = tri_corner(t, k);
            if (fresh >> cc & 1) {
                packed |= cc << (2 * n++);
                fresh &= ~(1 << cc);
            }
        }
    }
    *order = packed;
    return n;
}

__device__ __forceinline__ bool
point_thread(const PointViewDev *pv, int &v, int &x, int &y, size_t &p)
{
    v = blockIdx.y;
    PointViewDev const &P = pv[v];
    size_t const local = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (local >= (size_t)P.w * P.h)
        return false;
    x = (int)(local % P.w);
    y = (int)(local / P.w);
    p = P.off + local;
    return true;
}

__global__ void __launch_bounds__(256)
points_code_kernel(const MeshViewDev *__restrict__ views,
    const PointViewDev *__restrict__ pv, PointBufs B)
{
    int v, x, y;
    size_t p;
    if (!point_thread(pv, v, x, y, p))
        return;
    int c = 0;
    if (x < pv[v].w - 1 && y < pv[v].h - 1)
        c = block_code(views[v], pv[v].dm, x, y, B.dd_factor);
    B.code[p] = (uint8_t)c;
}

__global__ void __launch_bounds__(256)
points_count_kernel(const PointViewDev *__restrict__ pv, PointBufs B)
{
    int v, x, y;
    size_t p;
    if (!point_thread(pv, v, x, y, p))
        return;
    int const c = B.code[p];
    int order;
    int const nv = c ? block_new_corners(B.code + pv[v].off, pv[v].w, x, y, c, &order) : 0;
    int const nt = ((c & 7) != 0) + ((c >> 3) != 0);
    B.scan[p] = (unsigned long long)nv | (unsigned long long)nt << 32;
}

__global__ void __launch_bounds__(256)
points_vid_kernel(const PointViewDev *__restrict__ pv, PointBufs B)
{
    int v, x, y;
    size_t p;
    if (!point_thread(pv, v, x, y, p))
        return;
    int const c = B.code[p];
    if (c == 0)
        return;
    int const w = pv[v].w;
    int order;
    int const nv = block_new_corners(B.code + pv[v].off, w, x, y, c, &order);
    uint32_t const base = (uint32_t)B.scan[p];
    for (int r = 0; r < nv; ++r) {
        int const cc = order >> (2 * r) & 3;
        B.vid[p + (cc & 1) + (size_t)(cc >> 1) * w] = base + r;
    }
}

// direction code of a neighbour: (dy + 1) * 3 + (dx + 1), 4 = the pixel itself
__device__ __forceinline__ int
dir_offset(int d, int w)
{
    return (d / 3 - 1) * w + (d % 3 - 1);
}

// MeshInfo::update_vertex on the implicit mesh: the faces around pixel (x, y)
// in face-id order (blocks (x-1,y-1), (x,y-1), (x-1,y), (x,y); tri[0] before
// tri[1]), each as the edge (v1, v2) that follows the pixel in the face;
// chained front to back as std::list does; complex when some faces are left,
// then the neighbours sorted by vertex id
__global__ void __launch_bounds__(256)
points_topo_kernel(const PointViewDev *__restrict__ pv, PointBufs B)
{
    int v, x, y;
    size_t p;
    if (!point_thread(pv, v, x, y, p))
        return;
    int const w = pv[v].w;
    const uint8_t *code = B.code + pv[v].off;
    uint32_t e1 = 0, e2 = 0;   // nibble k: edge k's v1 / v2 direction
    int ne = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        int const bx = x - 1 + (b & 1), by = y - 1 + (b >> 1);
        if (bx < 0 || by < 0)
            continue;
        int const c = code[(size_t)by * w + bx];
        int const me = 3 - b;   // the pixel's corner in that block
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            int const t = (c >> (3 * j)) & 7;
            if (!(tri_mask(t) >> me & 1))
                continue;
            int k = 0;
            while (tri_corner(t, k) != me)
                ++k;
            int const c1 = tri_corner(t, (k + 1) % 3), c2 = tri_corner(t, (k + 2) % 3);
            // corner c of block b relative to the pixel: dx = (b & 1) - 1 + (c & 1)
            int const d1 = ((b >> 1) + (c1 >> 1)) * 3 + (b & 1) + (c1 & 1);
            int const d2 = ((b >> 1) + (c2 >> 1)) * 3 + (b & 1) + (c2 & 1);
            e1 |= (uint32_t)d1 << (4 * ne);
            e2 |= (uint32_t)d2 << (4 * ne);
            ++ne;
        }
    }
    if (ne == 0) {
        B.meta[p] = 0;
        B.dist[0][p] = 4;
        return;
    }
    // chain: edge indices as nibbles, front first
    uint32_t chain = 0;
    int len = 1;
    int front = e1 & 15, back = e2 & 15;
    int left = ((1 << ne) - 1) & ~1;
    while (left) {
        bool appended = false;
        for (int k = 1; k < 8; ++k) {
            if (!(left >> k & 1))
                continue;
            int const a = e1 >> (4 * k) & 15, bb = e2 >> (4 * k) & 15;
            if (a == back) {
                chain |= (uint32_t)k << (4 * len);
                back = bb;
            } else if (bb == front) {
                chain = chain << 4 | k;
                front = a;
            } else
                continue;
            ++len;
            left &= ~(1 << k);
            appended = true;
            break;
        }
        if (!appended)
            break;
    }
    uint32_t list = 0;
    int n = 0, border = 0;
    if (left) {
        // complex: every other vertex of the faces, sorted by vertex id
        int set = 0;
        for (int k = 0; k < ne; ++k)
            set |= 1 << (e1 >> (4 * k) & 15) | 1 << (e2 >> (4 * k) & 15);
        uint32_t ids[9];
#pragma unroll
        for (int d = 0; d < 9; ++d)
            ids[d] = (set >> d & 1) ? B.vid[p + dir_offset(d, w)] : 0xffffffffu;
        while (set) {
            int best = -1;
            uint32_t best_id = 0xffffffffu;
#pragma unroll
            for (int d = 0; d < 9; ++d)
                if ((set >> d & 1) && (best < 0 || ids[d] < best_id)) {
                    best = d;
                    best_id = ids[d];
                }
            list |= (uint32_t)best << (4 * n++);
            set &= ~(1 << best);
        }
    } else {
        for (int k = 0; k < len; ++k)
            list |= (e1 >> (4 * (chain >> (4 * k) & 15)) & 15) << (4 * n++);
        if (front != back) {
            border = 1;   // (at most 8 neighbours: the mesh is consistently oriented)
            list |= (uint32_t)back << (4 * n++);
        }
    }
    B.nbr[p] = list;
    B.meta[p] = (uint8_t)(n | border << 4 | 1 << 5);
    B.dist[0][p] = border ? 0 : 4;
}

// depthmap_mesh_confidences(m, 4): the rings grown from the border vertices
// give every vertex its hop distance d to the nearest one (the neighbour lists
// are symmetric), confidence min(d, 4) / 4; three rounds settle d <= 3
__global__ void __launch_bounds__(256)
points_ring_kernel(const PointViewDev *__restrict__ pv, PointBufs B, int src)
{
    int v, x, y;
    size_t p;
    if (!point_thread(pv, v, x, y, p))
        return;
    int const m = B.meta[p];
    int d = B.dist[src][p];
    if (m >> 5 & 1) {
        int const w = pv[v].w;
        uint32_t const list = B.nbr[p];
        for (int k = 0; k < (m & 15); ++k) {
            int const dn = B.dist[src][p + dir_offset(list >> (4 * k) & 15, w)] + 1;
            d = dn < d ? dn : d;
        }
    }
    B.dist[src ^ 1][p] = (uint8_t)d;
}

// MESH: the triangle mesh's vertices (M1 of DESIGN.md section 9.5): position,
// colour and confidence only; its normals come from mesh_normals_kernel
template <bool MESH>
__global__ void __launch_bounds__(256)
points_emit_kernel(const MeshViewDev *__restrict__ views,
    const PointViewDev *__restrict__ pv, PointBufs B, int dist_buf)
{
#pragma clang fp contract(off)
    int v, x, y;
    size_t p;
    if (!point_thread(pv, v, x, y, p))
        return;
    PointViewDev const &P = pv[v];
    MeshViewDev const &V = views[v];
    if (B.faces != nullptr) {
        int const c = B.code[p];
        if (c != 0) {
            uint32_t f = (uint32_t)(B.scan[p] >> 32);
            for (int j = 0; j < 2; ++j) {
                int const t = (c >> (3 * j)) & 7;
                if (t == 0)
                    continue;
                for (int k = 0; k < 3; ++k) {
                    int const cc = tri_corner(t, k);
                    B.faces[3 * (size_t)f + k] = B.vid[p + (cc & 1) + (size_t)(cc >> 1) * P.w];
                }
                ++f;
            }
        }
    }
    int const m = B.meta[p];
    if (!(m >> 5 & 1))
        return;
    size_t const id = B.vid[p];
    size_t const local = p - P.off;
    float pos[3];
    world_point(V, x, y, P.dm[local], pos);
    for (int r = 0; r < 3; ++r)
        B.xyz[3 * id + r] = pos[r];
    // colour: ci(i, 0..2), grey when fewer than 3 channels
    const uint8_t *px = P.image + local * P.channels;
    uint8_t const g = px[0];
    B.rgb[3 * id + 0] = g;
    B.rgb[3 * id + 1] = P.channels >= 3 ? px[1] : g;
    B.rgb[3 * id + 2] = P.channels >= 3 ? px[2] : g;
    int const d = B.dist[dist_buf][p];
    B.conf[id] = d >= 4 ? 1.0f : (float)d / 4.0f;
    if constexpr (MESH)
        return;
    // ViewProjection::get_proj, (int) truncation, lookup in the world-space
    // normal map; 0 where the reference leaves the value unset
    float const u = dot3(V.KR + 0, pos) - V.t[0];
    float const vv = dot3(V.KR + 3, pos) - V.t[1];
    float const ww = dot3(V.KR + 6, pos) - V.t[2];
    float const qx = u / ww, qy = vv / ww;
    float n[3] = { 0.0f, 0.0f, 0.0f };
    if (qx > -1.0f && qx < (float)P.w && qy > -1.0f && qy < (float)P.h) {
        size_t const q = (size_t)(int)qy * P.w + (int)qx;
        for (int r = 0; r < 3; ++r)
            n[r] = V.normals[3 * q + r];
    }
    for (int r = 0; r < 3; ++r)
        B.nrm[3 * id + r] = n[r];
    // mvscale: 2 * mean distance to the one-ring, in MeshInfo's order
    int const cnt = m & 15;
    uint32_t const list = B.nbr[p];
    float s = 0.0f;
    for (int k = 0; k < cnt; ++k) {
        int const dd = list >> (4 * k) & 15;
        int const nx = x + dd % 3 - 1, ny = y + dd / 3 - 1;
        float q[3], e[3];
        world_point(V, nx, ny, P.dm[(size_t)ny * P.w + nx], q);
        for (int r = 0; r < 3; ++r)
            e[r] = pos[r] - q[r];
        s += sqrtf(dot3(e, e));
    }
    s /= (float)cnt;
    s *= 2.0f;
    B.val[id] = s;
}

// ------------------------------------------------------------- triangle mesh
// smvsrecon --mesh: the faces survive the AABB clip
// (delete_vertices_fix_faces, M2) and every vertex gets recalc_normals' angle
// weighted normal (M3-M5).  A vertex belongs to one pixel and its faces lie in
// that pixel's four incident blocks, whose face ids grow in the order
// (x-1,y-1), (x,y-1), (x-1,y), (x,y), tri[0] before tri[1] (the topo pass's
// walk): gathering them in that order adds the same terms in the same order as
// the reference's scatter over the face list.  No atomics.
struct MeshClip {
    int on;
    float3 lo, hi;
};

// the global pixel of corner cc of block (bx, by) of a view starting at off
__device__ __forceinline__ size_t
corner_pixel(size_t off, int w, int bx, int by, int cc)
{
    return off + (size_t)(by + (cc >> 1)) * w + bx + (cc & 1);
}

// the vertex ids of triangle t of block (bx, by) and whether the clip keeps
// the face (M2 (a): every corner kept)
__device__ __forceinline__ bool
tri_vertices(const PointViewDev &P, const PointBufs &B, MeshClip clip, int bx, int by,
    int t, uint32_t *ids)
{
    bool keep = true;
    for (int k = 0; k < 3; ++k) {
        ids[k] = B.vid[corner_pixel(P.off, P.w, bx, by, tri_corner(t, k))];
        if (clip.on && outside_aabb(B.xyz + 3 * (size_t)ids[k], clip.lo, clip.hi))
            keep = false;
    }
    return keep;
}

// recalc_normals as a gather: the vertex of pixel p sums fn * w over its kept
// faces in face-id order, then normalises (M5); written to its pre-clip slot
__global__ void __launch_bounds__(256)
mesh_normals_kernel(const PointViewDev *__restrict__ pv, PointBufs B, MeshClip clip)
{
#pragma clang fp contract(off)
    int v, x, y;
    size_t p;
    if (!point_thread(pv, v, x, y, p))
        return;
    if (!(B.meta[p] >> 5 & 1))
        return;
    PointViewDev const &P = pv[v];
    float vn[3] = { 0.0f, 0.0f, 0.0f };
    for (int b = 0; b < 4; ++b) {
        int const bx = x - 1 + (b & 1), by = y - 1 + (b >> 1);
        if (bx < 0 || by < 0)
            continue;
        int const c = B.code[P.off + (size_t)by * P.w + bx];
        int const me = 3 - b;   // the pixel's corner in that block
        for (int j = 0; j < 2; ++j) {
            int const t = (c >> (3 * j)) & 7;
            if (!(tri_mask(t) >> me & 1))
                continue;
            uint32_t ids[3];
            if (!tri_vertices(P, B, clip, bx, by, t, ids))
                continue;
            float q[3][3];
            int k_me = 0;
            for (int k = 0; k < 3; ++k) {
                for (int r = 0; r < 3; ++r)
                    q[k][r] = B.xyz[3 * (size_t)ids[k] + r];
                if (tri_corner(t, k) == me)
                    k_me = k;
            }
            float fn[3], weight;
            if (!face_term(q, k_me, fn, &weight))
                continue;
            for (int r = 0; r < 3; ++r)
                vn[r] += fn[r] * weight;
        }
    }
    float const vnl = sqrtf(dot3(vn, vn));
    if (vnl > 0.0f)
        for (int r = 0; r < 3; ++r)
            vn[r] = vn[r] / vnl;
    size_t const id = B.vid[p];
    for (int r = 0; r < 3; ++r)
        B.nrm[3 * id + r] = vn[r];
}

// per block: the number of its faces the clip keeps (their order is the
// blocks' order, so an exclusive scan of these gives the new face ids)
__global__ void __launch_bounds__(256)
mesh_face_count_kernel(const PointViewDev *__restrict__ pv, PointBufs B, MeshClip clip,
    unsigned long long *__restrict__ count)
{
    int v, x, y;
    size_t p;
    if (!point_thread(pv, v, x, y, p))
        return;
    int const c = B.code[p];
    int n = 0;
    for (int j = 0; j < 2; ++j) {
        int const t = (c >> (3 * j)) & 7;
        uint32_t ids[3];
        if (t != 0 && tri_vertices(pv[v], B, clip, x, y, t, ids))
            ++n;
    }
    count[p] = (unsigned long long)n;
}

// M2 (b): the kept faces at their scanned position, vertex ids through the
// exclusive scan of the vertex keep flags (vmap)
__global__ void __launch_bounds__(256)
mesh_face_scatter_kernel(const PointViewDev *__restrict__ pv, PointBufs B, MeshClip clip,
    const unsigned long long *__restrict__ at, const unsigned long long *__restrict__ vmap,
    uint32_t *__restrict__ faces)
{
    int v, x, y;
    size_t p;
    if (!point_thread(pv, v, x, y, p))
        return;
    int const c = B.code[p];
    size_t f = (size_t)at[p];
    for (int j = 0; j < 2; ++j) {
        int const t = (c >> (3 * j)) & 7;
        uint32_t ids[3];
        if (t == 0 || !tri_vertices(pv[v], B, clip, x, y, t, ids))
            continue;
        for (int k = 0; k < 3; ++k)
            faces[3 * f + k] = (uint32_t)vmap[ids[k]];
        ++f;
    }
}

} // namespace smvs_hip

using namespace smvs_hip;

namespace {

// what smvs_points_generate and smvs_mesh_generate ask of export_views
struct ExportOptions {
    bool cut, use_aabb, want_faces, mesh;
    float aabb_min[3], aabb_max[3];
    float dd_factor;
};

int
export_views(int device, const smvs_point_view *views, int n_views,
    ExportOptions const &opt, smvs_points **handle, int64_t *n_points)
{
    SMVS_REQUIRE(handle != nullptr, "no handle pointer");
    *handle = nullptr;
    SMVS_REQUIRE(views != nullptr && n_views >= 1, "no views");
    SMVS_REQUIRE(n_views <= 4096, "too many views");
    SMVS_REQUIRE(opt.dd_factor >= 0.0f && std::isfinite(opt.dd_factor),
        "dd_factor must be finite and >= 0");
    size_t total_pix = 0;
    for (int i = 0; i < n_views; ++i) {
        smvs_point_view const &in = views[i];
        SMVS_REQUIRE(in.width > 0 && in.height > 0 && in.depth != nullptr
            && in.normals != nullptr && in.image != nullptr
            && in.channels >= 1 && in.channels <= 4 && in.flen > 0.0f, "bad view");
        total_pix += (size_t)in.width * in.height;
    }
    // vertex ids are 32-bit and the faces (<= 2 per pixel) as well
    SMVS_REQUIRE(total_pix < ((size_t)1 << 31), "too many pixels");
    bool const faces_out = opt.want_faces || opt.mesh;

    WorkspaceLease lease(device);
    if (lease.w == nullptr)
        return SMVS_ERR_HIP;
    Workspace &ws = *lease.w;
    Carver carve;
    ViewSlab s;
    carve_views(views, n_views, true, carve, s);
    size_t const ptable_at = carve(sizeof(PointViewDev) * n_views);
    size_t const N = total_pix;
    size_t const n_tiles = (N + SCAN_TILE - 1) / SCAN_TILE;
    size_t const code_at = carve(N), scan_at = carve(8 * N),
        tiles_at = carve(8 * (n_tiles + 1)), vid_at = carve(4 * N),
        nbr_at = carve(4 * N), meta_at = carve(N), dist0_at = carve(N),
        dist1_at = carve(N);
    // vertices (<= one per pixel): the output, and the stage of the AABB clip
    size_t out_at[2][5];
    for (int k = 0; k < (opt.use_aabb ? 2 : 1); ++k) {
        out_at[k][0] = carve(12 * N);
        out_at[k][1] = carve(12 * N);
        out_at[k][2] = carve(3 * N);
        out_at[k][3] = carve(4 * N);
        out_at[k][4] = opt.mesh ? 0 : carve(4 * N);
    }
    size_t const faces_at = faces_out ? carve(4 * 3 * 2 * N) : 0;
    // the clipped mesh: kept faces per block and their scan
    bool const clip_faces = opt.mesh && opt.use_aabb;
    size_t const fscan_at = clip_faces ? carve(8 * N) : 0;
    size_t const ftiles_at = clip_faces ? carve(8 * (n_tiles + 1)) : 0;
    char *slab = nullptr;
    int rc;
    if ((rc = ws.ensure(0, carve.total, &slab)) != SMVS_OK)
        return rc;
    hipStream_t const stream = ws.stream;
    if ((rc = upload_and_prepare(ws, slab, views, n_views, opt.cut, true, s)))
        return rc;
    MeshViewDev *const d_table = s.d_table;

    std::vector<PointViewDev> ptable(n_views);
    size_t off = 0;
    for (int i = 0; i < n_views; ++i) {
        MeshViewDev const &V = s.table[i];
        PointViewDev &P = ptable[i];
        P.w = V.w;
        P.h = V.h;
        P.channels = views[i].channels;
        P.off = off;
        // generate_mesh triangulates the cut maps, or the depth maps (:211-213)
        P.dm = opt.cut ? V.cut : V.depth_ray;
        P.image = s.images[i];
        off += (size_t)V.w * V.h;
    }
    PointViewDev *d_ptable = reinterpret_cast<PointViewDev *>(slab + ptable_at);
    if ((rc = ws.upload(d_ptable, ptable.data(), sizeof(PointViewDev) * n_views)))
        return rc;

    PointBufs B;
    B.code = reinterpret_cast<uint8_t *>(slab + code_at);
    B.scan = reinterpret_cast<unsigned long long *>(slab + scan_at);
    B.tiles = reinterpret_cast<unsigned long long *>(slab + tiles_at);
    B.vid = reinterpret_cast<uint32_t *>(slab + vid_at);
    B.nbr = reinterpret_cast<uint32_t *>(slab + nbr_at);
    B.meta = reinterpret_cast<uint8_t *>(slab + meta_at);
    B.dist[0] = reinterpret_cast<uint8_t *>(slab + dist0_at);
    B.dist[1] = reinterpret_cast<uint8_t *>(slab + dist1_at);
    auto outputs = [&](PointBufs &b, int k) {
        b.xyz = reinterpret_cast<float *>(slab + out_at[k][0]);
        b.nrm = reinterpret_cast<float *>(slab + out_at[k][1]);
        b.rgb = reinterpret_cast<uint8_t *>(slab + out_at[k][2]);
        b.conf = reinterpret_cast<float *>(slab + out_at[k][3]);
        b.val = opt.mesh ? nullptr : reinterpret_cast<float *>(slab + out_at[k][4]);
    };
    outputs(B, 0);
    uint32_t *const faces = faces_out ? reinterpret_cast<uint32_t *>(slab + faces_at) : nullptr;
    // with the clip the mesh's faces are written by the scatter below
    B.faces = clip_faces ? nullptr : faces;
    B.dd_factor = opt.dd_factor;
    MeshClip clip;
    clip.on = opt.use_aabb ? 1 : 0;
    clip.lo = make_float3(opt.aabb_min[0], opt.aabb_min[1], opt.aabb_min[2]);
    clip.hi = make_float3(opt.aabb_max[0], opt.aabb_max[1], opt.aabb_max[2]);

    dim3 const grid((unsigned)((s.max_pix + 255) / 256), (unsigned)n_views);
    hipLaunchKernelGGL(points_code_kernel, grid, dim3(256), 0, stream, d_table, d_ptable, B);
    hipLaunchKernelGGL(points_count_kernel, grid, dim3(256), 0, stream, d_ptable, B);
    SMVS_HIP_CHECK(hipGetLastError());
    if ((rc = exclusive_scan(stream, B.scan, N, B.tiles)))
        return rc;
    hipLaunchKernelGGL(points_vid_kernel, grid, dim3(256), 0, stream, d_ptable, B);
    hipLaunchKernelGGL(points_topo_kernel, grid, dim3(256), 0, stream, d_ptable, B);
    for (int r = 0; r < 3; ++r)
        hipLaunchKernelGGL(points_ring_kernel, grid, dim3(256), 0, stream, d_ptable, B, r & 1);
    if (opt.mesh) {
        hipLaunchKernelGGL(points_emit_kernel<true>, grid, dim3(256), 0, stream, d_table,
            d_ptable, B, 1);
        hipLaunchKernelGGL(mesh_normals_kernel, grid, dim3(256), 0, stream, d_ptable, B,
            clip);
    } else
        hipLaunchKernelGGL(points_emit_kernel<false>, grid, dim3(256), 0, stream, d_table,
            d_ptable, B, 1);
    SMVS_HIP_CHECK(hipGetLastError());
    unsigned long long sums = 0;
    if ((rc = ws.download(&sums, scan_total(B.tiles, N), sizeof(sums))))
        return rc;
    size_t n_vert = (size_t)(sums & 0xffffffffull);
    size_t n_face = (size_t)(sums >> 32);
    PointBufs O = B;
    if (opt.use_aabb && n_vert > 0) {
        outputs(O, 1);
        if ((rc = launch_aabb_clip(stream, n_vert, clip.lo, clip.hi, vertex_attrs(B),
                vertex_attrs(O), B.scan, B.tiles)))
            return rc;
        if (clip_faces) {
            unsigned long long *const fscan =
                reinterpret_cast<unsigned long long *>(slab + fscan_at);
            unsigned long long *const ftiles =
                reinterpret_cast<unsigned long long *>(slab + ftiles_at);
            hipLaunchKernelGGL(mesh_face_count_kernel, grid, dim3(256), 0, stream,
                d_ptable, B, clip, fscan);
            SMVS_HIP_CHECK(hipGetLastError());
            if ((rc = exclusive_scan(stream, fscan, N, ftiles)))
                return rc;
            hipLaunchKernelGGL(mesh_face_scatter_kernel, grid, dim3(256), 0, stream,
                d_ptable, B, clip, fscan, B.scan, faces);
            SMVS_HIP_CHECK(hipGetLastError());
            if ((rc = ws.download(&sums, scan_total(ftiles, N), sizeof(sums))))
                return rc;
            n_face = (size_t)sums;
        }
        if ((rc = ws.download(&sums, scan_total(B.tiles, n_vert), sizeof(sums))))
            return rc;
        n_vert = (size_t)sums;
    }
    for (int i = 0; i < n_views; ++i)
        if (views[i].cut_depth != nullptr
            && (rc = ws.download(views[i].cut_depth, ptable[i].dm,
                    sizeof(float) * s.table[i].w * s.table[i].h)))
            return rc;
    if ((rc = fill_points(ws, opt.mesh, false, n_vert, n_face, vertex_attrs(O), faces, nullptr,
            handle)))
        return rc;
    if (n_points != nullptr)
        *n_points = (*handle)->n_points;
    return SMVS_OK;
}

} // namespace

extern "C" int
smvs_points_generate(int device, const smvs_point_view *views, int n_views,
    const smvs_points_options *options, smvs_points **handle, int64_t *n_points)
{
    SMVS_REQUIRE(handle != nullptr, "no handle pointer");
    *handle = nullptr;
    smvs_points_options opt = { 1, 0, { 0, 0, 0 }, { 0, 0, 0 }, 5.0f, 0 };
    if (options != nullptr)
        opt = *options;
    SMVS_REQUIRE(!(opt.want_faces && opt.use_aabb),
        "the face list is not kept together with the AABB clip");
    ExportOptions e;
    e.cut = opt.cut_surfaces != 0;
    e.use_aabb = opt.use_aabb != 0;
    e.want_faces = opt.want_faces != 0;
    e.mesh = false;
    std::copy(opt.aabb_min, opt.aabb_min + 3, e.aabb_min);
    std::copy(opt.aabb_max, opt.aabb_max + 3, e.aabb_max);
    e.dd_factor = opt.dd_factor;
    return export_views(device, views, n_views, e, handle, n_points);
}

extern "C" int
smvs_mesh_generate(int device, const smvs_point_view *views, int n_views,
    const smvs_mesh_options *options, smvs_points **handle, int64_t *n_vertices,
    int64_t *n_faces)
{
    smvs_mesh_options opt = { 1, 0, { 0, 0, 0 }, { 0, 0, 0 }, 5.0f };
    if (options != nullptr)
        opt = *options;
    ExportOptions e;
    e.cut = opt.cut_surfaces != 0;
    e.use_aabb = opt.use_aabb != 0;
    e.want_faces = true;
    e.mesh = true;
    std::copy(opt.aabb_min, opt.aabb_min + 3, e.aabb_min);
    std::copy(opt.aabb_max, opt.aabb_max + 3, e.aabb_max);
    e.dd_factor = opt.dd_factor;
    int const rc = export_views(device, views, n_views, e, handle, n_vertices);
    if (rc == SMVS_OK && n_faces != nullptr)
        *n_faces = (*handle)->n_faces;
    return rc;
}

