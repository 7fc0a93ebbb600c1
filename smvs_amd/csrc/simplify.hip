// smvsrecon --simplify on gfx950:
// DepthTriangulator::approximate_triangulation (lib/depth_triangulator.cc:27-305)
// over Delaunay2D (lib/delaunay_2d.cc, lib/quad_edge.h) for every view, then the
// export of mesh.hip's entries on the irregular meshes.  The view stage, the
// vertex clip and the result fill are the shared ones of export_shared.h.
//
//   greedy   one persistent workgroup per view runs the whole insertion loop:
//            selection (all lanes: max key, earliest scan stamp), the Delaunay
//            update (one lane, quad-edges as 32-bit indices in the view's
//            arena), the rescan of the changed triangles (a wave per small
//            triangle, the workgroup for a large one)
//   clean    per view: S9-S12 (corner deletion, colours, world positions, bad
//            faces, delete_invalid_faces' permutation, unreferenced vertices)
//   attrs    per view: face lists per vertex in face-id order, MeshInfo's
//            chained one-ring, the confidence rings, then position, colour,
//            confidence and value + looked-up normal (or recalc_normals'
//            gather) written at the view's offset in the merged mesh
//   clip     keep flags, scan, order-preserving compaction (AABB only)
//
// Arithmetic in the stated order, FMA contraction off.  Every walk over the
// subdivision has an iteration cap; hitting one ends the view with a status the
// entry returns.
#include "common.h"
#include "export_shared.h"
#include "mesh_shared.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <vector>

namespace smvs_hip {

enum { R_STATUS = 0, R_ITER, R_NVERT, R_NTRI, R_OUT_V, R_OUT_F, R_NUM = 8 };
enum { SIMP_OK = 0, SIMP_WALK_CAP = 1, SIMP_ARENA = 2, SIMP_ROWS = 3 };
constexpr int SIMP_THREADS = 256, SIMP_MAX_ROWS = 4100;

struct SimpView {
    int w, h, channels, budget;
    double max_error;           // < 0: S2's default
    const float *dm;            // the triangulated map
    const uint8_t *image;
    // the greedy loop's arena
    int max_edges, max_tris, max_verts;
    double *verts;              // [max_verts][3]
    uint32_t *next, *datum;     // [4 * max_edges] quarter-edges
    uint32_t *tri_start;        // [max_tris]
    double *tri_key;
    uint32_t *tri_stamp;
    float *tri_cand;            // [max_tris][3]
    int *tri_nzero;
    uint32_t *changed;          // [max_tris]
    int *result;                // [R_NUM]
    unsigned long long *clocks; // [4]: select, delaunay, scan, total (100 MHz ticks)
    // clean-up and attributes
    float *pos0, *pos;          // [max_verts][3]
    uint8_t *rgb0, *rgb;
    uint32_t *f1, *f2;          // [max_tris][3]
    uint32_t *sa, *sb;          // [max_tris + 1] scratch
    uint32_t *vmap;             // [max_verts + 1]
    uint32_t *adj_off, *adj_cnt;    // [max_verts + 1]
    uint32_t *adj;              // [3 * max_tris]
    uint32_t *nbr;              // [6 * max_tris]
    uint32_t *nbr_at, *nbr_cnt; // [max_verts]
    uint8_t *dist[2];           // [max_verts]
    uint8_t *vflag;             // [max_verts]
    size_t out_v, out_f;        // the view's offsets in the merged mesh
};

// ------------------------------------------------------------------ S4: tools
__device__ __forceinline__ double
area2(double ax, double ay, double bx, double by, double cx, double cy)
{
#pragma clang fp contract(off)
    return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
}

__device__ __forceinline__ double
sqn2(double x, double y)
{
#pragma clang fp contract(off)
    double s = 0.0;
    s += x * x;
    s += y * y;
    return s;
}

struct Quads {
    uint32_t *next, *datum;
    const double *verts;

    __device__ static uint32_t rot(uint32_t e, uint32_t k) { return (e & ~3u) | ((e + k) & 3u); }
    __device__ static uint32_t inv(uint32_t e) { return rot(e, 2); }
    __device__ uint32_t onext(uint32_t e) const { return next[e]; }
    __device__ uint32_t oprev(uint32_t e) const { return rot(next[rot(e, 1)], 1); }
    __device__ uint32_t dprev(uint32_t e) const { return rot(next[rot(e, 3)], 3); }
    __device__ uint32_t lnext(uint32_t e) const { return rot(next[rot(e, 3)], 1); }
    __device__ uint32_t lprev(uint32_t e) const { return inv(next[e]); }
    __device__ uint32_t orig(uint32_t e) const { return datum[e]; }
    __device__ uint32_t dest(uint32_t e) const { return datum[inv(e)]; }
    __device__ uint32_t left(uint32_t e) const { return datum[rot(e, 1)]; }
    __device__ uint32_t right(uint32_t e) const { return datum[rot(e, 3)]; }
    __device__ void set_left(uint32_t e, uint32_t f) { datum[rot(e, 1)] = f; }
    __device__ void set_right(uint32_t e, uint32_t f) { datum[rot(e, 3)] = f; }
    __device__ void set_ends(uint32_t e, uint32_t o, uint32_t d)
    {
        datum[e] = o;
        datum[inv(e)] = d;
    }
    __device__ void splice(uint32_t a, uint32_t b)
    {
        uint32_t const alpha = rot(next[a], 1), beta = rot(next[b], 1);
        uint32_t const an = next[a], bn = next[b], aln = next[alpha], ben = next[beta];
        next[a] = bn;
        next[b] = an;
        next[alpha] = ben;
        next[beta] = aln;
    }
    // is vertex p right of the edge e (orig -> dest)
    __device__ bool right_of(double px, double py, uint32_t e) const
    {
        const double *o = verts + 3 * (size_t)orig(e), *d = verts + 3 * (size_t)dest(e);
        return area2(px, py, d[0], d[1], o[0], o[1]) > 0;
    }
};

// The state of one view's subdivision while its lane works on it
struct Delaunay {
    Quads q;
    double *verts;
    uint32_t *tri_start, *changed;
    int n_edges, n_verts, n_tris, n_changed;
    int max_edges, max_verts, max_tris;

    __device__ uint32_t make_edge()
    {
        uint32_t const e = 4u * (uint32_t)n_edges++;
        q.next[e] = e;
        q.next[e + 1] = e + 3;
        q.next[e + 2] = e + 2;
        q.next[e + 3] = e + 1;
        for (int k = 0; k < 4; ++k)
            q.datum[e + k] = 0;
        return e;
    }
    __device__ uint32_t connect(uint32_t a, uint32_t b)
    {
        uint32_t const e = make_edge();
        q.splice(e, q.lnext(a));
        q.splice(Quads::inv(e), b);
        q.set_ends(e, q.dest(a), q.orig(b));
        return e;
    }
    // std::set::insert
    __device__ void mark(uint32_t id)
    {
        int at = 0;
        while (at < n_changed && changed[at] < id)
            ++at;
        if (at < n_changed && changed[at] == id)
            return;
        for (int k = n_changed; k > at; --k)
            changed[k] = changed[k - 1];
        changed[at] = id;
        ++n_changed;
    }
    __device__ void flip(uint32_t e)
    {
        uint32_t const a = q.oprev(e), b = q.oprev(Quads::inv(e));
        q.splice(e, a);
        q.splice(Quads::inv(e), b);
        q.splice(e, q.lnext(a));
        q.splice(Quads::inv(e), q.lnext(b));
        q.set_ends(e, q.dest(a), q.dest(b));
        uint32_t const lf = q.left(e), rf = q.right(e);
        q.set_left(q.lnext(e), lf);
        q.set_left(q.lprev(e), lf);
        q.set_left(Quads::inv(q.next[Quads::inv(e)]), rf);
        q.set_left(q.oprev(e), rf);
        tri_start[lf] = e;
        tri_start[rf] = Quads::inv(e);
        mark(lf);
        mark(rf);
    }
    __device__ void initialize(const double *corners)
    {
        for (int k = 0; k < 12; ++k)
            verts[k] = corners[k];
        n_verts = 4;
        uint32_t const e1 = make_edge();
        q.set_ends(e1, 0, 1);
        uint32_t const e2 = make_edge();
        q.splice(Quads::inv(e1), e2);
        q.set_ends(e2, 1, 2);
        uint32_t const e3 = make_edge();
        q.splice(Quads::inv(e2), e3);
        q.set_ends(e3, 2, 0);
        q.splice(Quads::inv(e3), e1);
        tri_start[0] = e1;
        q.set_left(e1, 0);
        q.set_left(e2, 0);
        q.set_left(e3, 0);
        uint32_t const e4 = make_edge();
        q.splice(Quads::inv(e1), e4);
        q.set_ends(e4, 1, 3);
        uint32_t const e5 = make_edge();
        q.splice(Quads::inv(e4), e5);
        q.set_ends(e5, 3, 2);
        q.splice(Quads::inv(e5), Quads::inv(e2));
        tri_start[1] = e4;
        q.set_left(e4, 1);
        q.set_left(e5, 1);
        uint32_t const c = q.lnext(e5);
        q.set_left(c, 1);
        q.set_right(Quads::inv(c), 1);
        n_tris = 2;
    }
    // -> SIMP_OK, or the reason the view ends
    __device__ int insert(double px, double py, double pz, uint32_t triangle)
    {
#pragma clang fp contract(off)
        n_changed = 0;
        if (n_edges + 4 > max_edges || n_verts + 1 > max_verts || n_tris + 2 > max_tris)
            return SIMP_ARENA;
        int const cap = 8 * n_edges + 64;
        uint32_t e = tri_start[triangle];
        int steps = 0;
        for (;; ++steps) {
            if (steps > cap)
                return SIMP_WALK_CAP;
            const double *o = verts + 3 * (size_t)q.orig(e), *d = verts + 3 * (size_t)q.dest(e);
            if ((px == o[0] && py == o[1]) || (px == d[0] && py == d[1]))
                return SIMP_OK;   // S5: p is a vertex already
            if (q.right_of(px, py, e)) {
                e = Quads::inv(e);
                continue;
            }
            uint32_t const n = q.onext(e);
            if (!q.right_of(px, py, n)) {
                e = n;
                continue;
            }
            uint32_t const dp = q.dprev(e);
            if (!q.right_of(px, py, dp)) {
                e = dp;
                continue;
            }
            break;
        }
        {
            // on_edge, eps 1e-5
            const double *o = verts + 3 * (size_t)q.orig(e), *d = verts + 3 * (size_t)q.dest(e);
            double const eps = 1e-5;
            double const t1 = sqrt(sqn2(px - o[0], py - o[1]));
            double const t2 = sqrt(sqn2(px - d[0], py - d[1]));
            bool on = false;
            if (t1 < eps || t2 < eps)
                on = true;
            else {
                double const t3 = sqrt(sqn2(o[0] - d[0], o[1] - d[1]));
                if (!(t1 > t3 || t2 > t3)) {
                    double dist = ((d[1] - o[1]) * px) - ((d[0] - o[0]) * py) + d[0] * o[1]
                        - d[1] * o[0];
                    dist /= t3;
                    on = fabs(dist) < eps;
                }
            }
            if (on) {
                e = q.oprev(e);
                uint32_t const gone = q.onext(e);
                q.splice(gone, q.oprev(gone));
                q.splice(Quads::inv(gone), q.oprev(Quads::inv(gone)));
            }
        }
        uint32_t base = make_edge();
        uint32_t const pv = (uint32_t)n_verts++;
        verts[3 * (size_t)pv] = px;
        verts[3 * (size_t)pv + 1] = py;
        verts[3 * (size_t)pv + 2] = pz;
        q.set_ends(base, q.orig(e), pv);
        q.set_right(base, q.left(e));
        tri_start[q.left(e)] = e;
        mark(q.left(e));
        q.splice(base, e);
        uint32_t const first = base;
        for (int i = 0; i < 2; ++i) {
            base = connect(e, Quads::inv(base));
            q.set_left(base, q.left(e));
            e = q.oprev(base);
            uint32_t const t = (uint32_t)n_tris++;
            tri_start[t] = e;
            mark(t);
            q.set_left(e, t);
            q.set_right(base, t);
        }
        if (q.lnext(e) != first) {
            base = connect(e, Quads::inv(base));
            q.set_left(base, q.left(e));
            e = q.oprev(base);
            tri_start[q.left(e)] = e;
            mark(q.left(e));
            q.set_right(base, q.left(e));
        }
        q.set_left(first, q.left(e));
        for (steps = 0;; ++steps) {
            if (steps > cap)
                return SIMP_WALK_CAP;
            uint32_t const t = q.oprev(e);
            const double *o = verts + 3 * (size_t)q.orig(e), *d = verts + 3 * (size_t)q.dest(e),
                *c = verts + 3 * (size_t)q.dest(t);
            bool swap = area2(c[0], c[1], d[0], d[1], o[0], o[1]) > 0;
            if (swap) {
                // in_circle(orig(e), dest(t), dest(e), p)
                double const v = sqn2(o[0], o[1]) * area2(c[0], c[1], d[0], d[1], px, py)
                    - sqn2(c[0], c[1]) * area2(o[0], o[1], d[0], d[1], px, py)
                    + sqn2(d[0], d[1]) * area2(o[0], o[1], c[0], c[1], px, py)
                    - sqn2(px, py) * area2(o[0], o[1], c[0], c[1], d[0], d[1]);
                swap = v > 0;
            }
            if (swap) {
                if (n_changed + 2 > max_tris)
                    return SIMP_ARENA;
                flip(e);
                e = q.oprev(e);
            } else if (q.onext(e) == first)
                return SIMP_OK;
            else
                e = q.lprev(q.onext(e));
        }
    }
};

// ---------------------------------------------------------------- S7 / S8
// What every lane needs to rescan a triangle: the plane and the two parts of
// the rasteriser (rows upward from (xa, ya), then rows downward from (xb, yb)).
struct TriScan {
    double n0, n1, n2, d;
    double xa, da1, da2, xb, db1, db2;
    int ya, na, yb, nb;
};

__device__ void
tri_scan_setup(SimpView const &V, uint32_t id, TriScan &S)
{
#pragma clang fp contract(off)
    Quads q{ V.next, V.datum, V.verts };
    double p[3][3];
    uint32_t e = V.tri_start[id];
    for (int k = 0; k < 3; ++k) {
        const double *v = V.verts + 3 * (size_t)q.orig(e);
        p[k][0] = v[0];
        p[k][1] = v[1];
        p[k][2] = v[2];
        e = q.lprev(e);
    }
    double const ux = p[1][0] - p[0][0], uy = p[1][1] - p[0][1], uz = p[1][2] - p[0][2];
    double const vx = p[2][0] - p[0][0], vy = p[2][1] - p[0][1], vz = p[2][2] - p[0][2];
    double n[3] = { uy * vz - uz * vy, uz * vx - ux * vz, ux * vy - uy * vx };
    double len = 0.0;
    len += n[0] * n[0];
    len += n[1] * n[1];
    len += n[2] * n[2];
    len = sqrt(len);
    for (int k = 0; k < 3; ++k)
        n[k] = n[k] / len;
    double dot = 0.0;
    dot += p[0][0] * n[0];
    dot += p[0][1] * n[1];
    dot += p[0][2] * n[2];
    S.n0 = n[0];
    S.n1 = n[1];
    S.n2 = n[2];
    S.d = -dot;
    // stable sort by y
    double sx[3] = { p[0][0], p[1][0], p[2][0] }, sy[3] = { p[0][1], p[1][1], p[2][1] };
    for (int i = 1; i < 3; ++i)
        for (int j = i; j > 0 && sy[j] < sy[j - 1]; --j) {
            double t = sx[j]; sx[j] = sx[j - 1]; sx[j - 1] = t;
            t = sy[j]; sy[j] = sy[j - 1]; sy[j - 1] = t;
        }
    S.na = S.nb = 0;
    S.xa = S.da1 = S.da2 = S.xb = S.db1 = S.db2 = 0.0;
    S.ya = S.yb = 0;
    auto top_flat = [&](double ax, double ay, double bx, double by, double cx, double cy) {
        S.da1 = (ax - cx) / (ay - cy);
        S.da2 = (ax - bx) / (ay - by);
        S.xa = ax;
        S.ya = (int)ay;
        S.na = (int)floor(by) - S.ya + 1;
    };
    auto bottom_flat = [&](double ax, double ay, double bx, double by, double cx, double cy) {
        S.db1 = (cx - ax) / (cy - ay);
        S.db2 = (cx - bx) / (cy - by);
        S.xb = cx;
        S.yb = (int)cy;
        S.nb = S.yb - (int)floor(by);
    };
    if (sy[1] == sy[2])
        top_flat(sx[0], sy[0], sx[1], sy[1], sx[2], sy[2]);
    else if (sy[0] == sy[1])
        bottom_flat(sx[0], sy[0], sx[1], sy[1], sx[2], sy[2]);
    else {
        double mx = sx[0] + ((sy[1] - sy[0]) / (sy[2] - sy[0])) * (sx[2] - sx[0]);
        mx = sx[0] < sx[1] ? ceil(mx) : floor(mx);
        top_flat(sx[0], sy[0], sx[1], sy[1], mx, sy[1]);
        bottom_flat(sx[1], sy[1], mx, sy[1], sx[2], sy[2]);
    }
    S.na = S.na < 0 ? 0 : S.na;
    S.nb = S.nb < 0 ? 0 : S.nb;
}

// the span of row r in emission order, clamped to the map: -> y, xs, xe
// (xs > xe: nothing to visit)
__device__ __forceinline__ void
row_span_from(SimpView const &V, double x1, double x2, int y, int &xs, int &xe)
{
    double const lo = x2 < x1 ? x2 : x1, hi = x1 < x2 ? x2 : x1;
    double const cl = ceil(lo), fh = floor(hi);
    // (the clamp drops only pixels S7 skips as outside the map)
    xs = cl > 0.0 ? (cl < 8192.0 ? (int)cl : 8192) : 0;
    xe = fh < (double)(V.w - 1) ? (fh > -1.0 ? (int)fh : -1) : V.w - 1;
    if (y < 0 || y > V.h - 1 || !(lo == lo) || !(hi == hi))
        xe = -1, xs = 0;
}

__device__ void
row_span(SimpView const &V, TriScan const &S, int r, int &y, int &xs, int &xe)
{
#pragma clang fp contract(off)
    double x1, x2;
    if (r < S.na) {
        x1 = x2 = S.xa;
        for (int k = 0; k < r; ++k) {
            x1 += S.da1;
            x2 += S.da2;
        }
        y = S.ya + r;
    } else {
        int const kk = r - S.na;
        x1 = x2 = S.xb;
        for (int k = 0; k < kk; ++k) {
            x1 -= S.db1;
            x2 -= S.db2;
        }
        y = S.yb - kk;
    }
    row_span_from(V, x1, x2, y, xs, xe);
}

struct ScanBest {
    double dist;
    uint32_t key;   // row << 13 | x: the position in S8's order
    int zeros;
};

__device__ __forceinline__ void
scan_pixel(SimpView const &V, TriScan const &S, int r, int x, int y, ScanBest &b)
{
#pragma clang fp contract(off)
    float const depth = V.dm[(size_t)y * V.w + x];
    if (depth == 0.0f) {
        ++b.zeros;
        return;
    }
    double const dist = fabs(S.n0 * (double)x + S.n1 * (double)y + S.n2 * (double)depth + S.d);
    uint32_t const key = (uint32_t)r << 13 | (uint32_t)x;
    if (dist > b.dist || (dist == b.dist && dist > 0.0 && key < b.key)) {
        b.dist = dist;
        b.key = key;
    }
}

__device__ __forceinline__ void
scan_merge(ScanBest &a, double dist, uint32_t key, int zeros)
{
    if (dist > a.dist || (dist == a.dist && key < a.key)) {
        a.dist = dist;
        a.key = key;
    }
    a.zeros += zeros;
}

__device__ __forceinline__ void
wave_reduce_best(ScanBest &b)
{
    for (int o = 32; o > 0; o >>= 1) {
        double const d = __shfl_xor(b.dist, o, 64);
        uint32_t const k = __shfl_xor(b.key, o, 64);
        int const z = __shfl_xor(b.zeros, o, 64);
        scan_merge(b, d, k, z);
    }
}

__device__ void
scan_store(SimpView const &V, TriScan const &S, uint32_t id, ScanBest const &b, uint32_t stamp)
{
    float cx = 0.0f, cy = 0.0f, cz = 0.0f;
    if (b.dist > 0.0) {
        int const r = (int)(b.key >> 13), x = (int)(b.key & 8191u);
        int const y = r < S.na ? S.ya + r : S.yb - (r - S.na);
        cx = (float)x;
        cy = (float)y;
        cz = V.dm[(size_t)y * V.w + x];
    }
    V.tri_key[id] = b.dist;
    V.tri_cand[3 * (size_t)id] = cx;
    V.tri_cand[3 * (size_t)id + 1] = cy;
    V.tri_cand[3 * (size_t)id + 2] = cz;
    V.tri_nzero[id] = b.zeros;
    V.tri_stamp[id] = stamp;
}

// a small triangle (<= 64 rows) by one wave: lane r runs row r's recurrence
__device__ void
scan_triangle_wave(SimpView const &V, TriScan const &S, uint32_t id, uint32_t stamp)
{
    int const lane = threadIdx.x & 63;
    int const rows = S.na + S.nb;
    int y = 0, xs = 0, xe = -1;
    if (lane < rows)
        row_span(V, S, lane, y, xs, xe);
    ScanBest b{ 0.0, 0xffffffffu, 0 };
    for (int r = 0; r < rows; ++r) {
        int const ry = __shfl(y, r, 64), rs = __shfl(xs, r, 64), re = __shfl(xe, r, 64);
        for (int x = rs + lane; x <= re; x += 64)
            scan_pixel(V, S, r, x, ry, b);
    }
    wave_reduce_best(b);
    if (lane == 0)
        scan_store(V, S, id, b, stamp);
}

// a large triangle by the workgroup: the spans by a serial pass into LDS
__device__ void
scan_triangle_block(SimpView const &V, TriScan const &S, uint32_t id, uint32_t stamp,
    int2 *s_rows, ScanBest *s_best)
{
#pragma clang fp contract(off)
    int const tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int const rows = S.na + S.nb;
    if (tid == 0) {
        double x1 = S.xa, x2 = S.xa;
        for (int r = 0; r < S.na; ++r) {
            int xs, xe;
            row_span_from(V, x1, x2, S.ya + r, xs, xe);
            s_rows[r] = make_int2(xs, xe);
            x1 += S.da1;
            x2 += S.da2;
        }
        x1 = x2 = S.xb;
        for (int r = 0; r < S.nb; ++r) {
            int xs, xe;
            row_span_from(V, x1, x2, S.yb - r, xs, xe);
            s_rows[S.na + r] = make_int2(xs, xe);
            x1 -= S.db1;
            x2 -= S.db2;
        }
    }
    __syncthreads();
    ScanBest b{ 0.0, 0xffffffffu, 0 };
    for (int r = wave; r < rows; r += SIMP_THREADS / 64) {
        int2 const span = s_rows[r];
        int const y = r < S.na ? S.ya + r : S.yb - (r - S.na);
        for (int x = span.x + lane; x <= span.y; x += 64)
            scan_pixel(V, S, r, x, y, b);
    }
    wave_reduce_best(b);
    if (lane == 0)
        s_best[wave] = b;
    __syncthreads();
    if (tid == 0) {
        ScanBest t = s_best[0];
        for (int k = 1; k < SIMP_THREADS / 64; ++k)
            scan_merge(t, s_best[k].dist, s_best[k].key, s_best[k].zeros);
        scan_store(V, S, id, t, stamp);
    }
    __syncthreads();
}

// S1-S8: the whole loop of one view.  STAMPS: the diagnostic build that
// splits the loop's time (smvs_simplify_triangulate with clocks4); the export
// runs the build without a clock read.
template <bool STAMPS>
__global__ void __launch_bounds__(SIMP_THREADS)
simplify_greedy_kernel(const SimpView *__restrict__ views)
{
#pragma clang fp contract(off)
    SimpView const V = views[blockIdx.x];
    int const tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __shared__ int2 s_rows[SIMP_MAX_ROWS];
    __shared__ ScanBest s_best[SIMP_THREADS / 64];
    __shared__ float s_chunk[4 * SIMP_THREADS];
    __shared__ float s_fmax[SIMP_THREADS / 64];
    __shared__ double s_key[SIMP_THREADS / 64];
    __shared__ uint32_t s_stamp[SIMP_THREADS / 64], s_id[SIMP_THREADS / 64];
    __shared__ int s_state[4];   // status, changed, triangles
    __shared__ double s_max_error;
    __shared__ Delaunay s_del;
    size_t const npix = (size_t)V.w * V.h;
    unsigned long long t_sel = 0, t_del = 0, t_scan = 0, t0 = STAMPS ? wall_clock64() : 0;

    // S2: dm_max (any order), the float sum in memory order (one lane, fed from LDS)
    float mx = V.dm[0];
    for (size_t i = tid; i < npix; i += SIMP_THREADS)
        mx = fmaxf(mx, V.dm[i]);
    for (int o = 32; o > 0; o >>= 1)
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    if (lane == 0)
        s_fmax[wave] = mx;
    float avg = 0.0f, counter = 0.0f;
    for (size_t at = 0; at < npix; at += 4 * SIMP_THREADS) {
        __syncthreads();
        for (int k = 0; k < 4; ++k) {
            size_t const i = at + (size_t)k * SIMP_THREADS + tid;
            s_chunk[k * SIMP_THREADS + tid] = i < npix ? V.dm[i] : 0.0f;
        }
        __syncthreads();
        if (tid == 0) {
#pragma unroll 8
            for (int k = 0; k < 4 * SIMP_THREADS; ++k) {
                float const v = s_chunk[k];
                if (v > 0.0f) {
                    avg += v;
                    counter += 1.0f;
                }
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        float dm_max = s_fmax[0];
        for (int k = 1; k < SIMP_THREADS / 64; ++k)
            dm_max = fmaxf(dm_max, s_fmax[k]);
        avg /= counter;
        double max_error = V.max_error;
        if (max_error < 0.0)
            max_error = (double)(dm_max - avg) * 1e-3;
        s_max_error = max_error;
        // S3
        double corners[12];
        int const cx[4] = { 0, V.w - 1, 0, V.w - 1 }, cy[4] = { 0, 0, V.h - 1, V.h - 1 };
        for (int k = 0; k < 4; ++k) {
            float const d = V.dm[(size_t)cy[k] * V.w + cx[k]];
            corners[3 * k] = (k & 1) ? (double)V.w : -1.0;
            corners[3 * k + 1] = (k & 2) ? (double)V.h : -1.0;
            corners[3 * k + 2] = d > 0.0f ? (double)d : (double)dm_max;
        }
        Delaunay &D = s_del;
        D.q = Quads{ V.next, V.datum, V.verts };
        D.verts = V.verts;
        D.tri_start = V.tri_start;
        D.changed = V.changed;
        D.n_edges = D.n_verts = D.n_tris = D.n_changed = 0;
        D.max_edges = V.max_edges;
        D.max_verts = V.max_verts;
        D.max_tris = V.max_tris;
        D.initialize(corners);
        V.changed[0] = 0;
        V.changed[1] = 1;
        s_state[0] = SIMP_OK;
        s_state[1] = 2;
        s_state[2] = 2;
    }
    __threadfence_block();
    __syncthreads();

    uint32_t stamp = 0;
    int iterations = 0;
    bool first = true;
    for (;;) {
        // ---- rescan the changed triangles in ascending order (S6)
        unsigned long long const c0 = STAMPS ? wall_clock64() : 0;
        int const n_changed = s_state[1];
        int small = 0;
        for (int j = 0; j < n_changed; ++j) {
            uint32_t const id = V.changed[j];
            TriScan S;
            tri_scan_setup(V, id, S);
            int const rows = S.na + S.nb;
            if (rows > SIMP_MAX_ROWS) {
                if (tid == 0)
                    s_state[0] = SIMP_ROWS;
            } else if (rows > 64)
                scan_triangle_block(V, S, id, stamp + j, s_rows, s_best);
            else if ((small++ & 3) == wave)
                scan_triangle_wave(V, S, id, stamp + j);
        }
        stamp += (uint32_t)n_changed;
        __threadfence_block();
        __syncthreads();
        unsigned long long const c1 = STAMPS ? wall_clock64() : 0;
        t_scan += c1 - c0;
        if (s_state[0] != SIMP_OK)
            break;
        if (!first && n_changed == 0) {
            // S5: nothing changed, so every further iteration repeats this one
            iterations = V.budget;
            break;
        }
        first = false;
        if (iterations >= V.budget)
            break;
        // ---- selection: the largest key, the earliest stamp among equals
        int const n_tris = s_state[2];
        double bk = -1.0;
        uint32_t bs = 0xffffffffu, bi = 0;
        for (int t = tid; t < n_tris; t += SIMP_THREADS) {
            double const k = V.tri_key[t];
            uint32_t const s = V.tri_stamp[t];
            if (k > bk || (k == bk && s < bs)) {
                bk = k;
                bs = s;
                bi = (uint32_t)t;
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            double const k = __shfl_xor(bk, o, 64);
            uint32_t const s = __shfl_xor(bs, o, 64), i = __shfl_xor(bi, o, 64);
            if (k > bk || (k == bk && s < bs)) {
                bk = k;
                bs = s;
                bi = i;
            }
        }
        if (lane == 0) {
            s_key[wave] = bk;
            s_stamp[wave] = bs;
            s_id[wave] = bi;
        }
        __syncthreads();
        bk = s_key[0];
        bs = s_stamp[0];
        bi = s_id[0];
        for (int k = 1; k < SIMP_THREADS / 64; ++k)
            if (s_key[k] > bk || (s_key[k] == bk && s_stamp[k] < bs)) {
                bk = s_key[k];
                bs = s_stamp[k];
                bi = s_id[k];
            }
        unsigned long long const c2 = STAMPS ? wall_clock64() : 0;
        t_sel += c2 - c1;
        if (bk < s_max_error)
            break;
        ++iterations;
        // ---- the Delaunay update, one lane
        if (tid == 0) {
            Delaunay &D = s_del;
            const float *c = V.tri_cand + 3 * (size_t)bi;
            int const rc = D.insert((double)c[0], (double)c[1], (double)c[2], bi);
            s_state[0] = rc;
            s_state[1] = D.n_changed;
            s_state[2] = D.n_tris;
        }
        __threadfence_block();
        __syncthreads();
        t_del += (STAMPS ? wall_clock64() : 0) - c2;
        if (s_state[0] != SIMP_OK)
            break;
    }
    if (tid == 0) {
        V.result[R_STATUS] = s_state[0];
        V.result[R_ITER] = iterations;
        V.result[R_NVERT] = s_del.n_verts;
        V.result[R_NTRI] = s_del.n_tris;
        V.clocks[0] = t_sel;
        V.clocks[1] = t_del;
        V.clocks[2] = t_scan;
        V.clocks[3] = (STAMPS ? wall_clock64() : 0) - t0;
    }
}

// ------------------------------------------------------------ workgroup scan
// exclusive scan of a[0..n) in place by the whole workgroup -> the total
__device__ uint32_t
block_scan_u32(uint32_t *a, int n)
{
    __shared__ uint32_t s_w[SIMP_THREADS / 64];
    int const tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t carry = 0;
    for (int base = 0; base < n; base += SIMP_THREADS) {
        int const i = base + tid;
        uint32_t const v = i < n ? a[i] : 0u;
        uint32_t inc = v;
        for (int o = 1; o < 64; o <<= 1) {
            uint32_t const t = __shfl_up(inc, o, 64);
            if (lane >= o)
                inc += t;
        }
        if (lane == 63)
            s_w[wave] = inc;
        __syncthreads();
        uint32_t pre = 0, tot = 0;
        for (int k = 0; k < SIMP_THREADS / 64; ++k) {
            pre += k < wave ? s_w[k] : 0u;
            tot += s_w[k];
        }
        __syncthreads();
        if (i < n)
            a[i] = carry + pre + inc - v;
        carry += tot;
    }
    __threadfence_block();
    __syncthreads();
    return carry;
}

__device__ __forceinline__ float
edge_length(const float *p, uint32_t a, uint32_t b)
{
#pragma clang fp contract(off)
    float e[3];
    for (int r = 0; r < 3; ++r)
        e[r] = p[3 * (size_t)a + r] - p[3 * (size_t)b + r];
    return sqrtf(dot3(e, e));
}

// S9-S12 for one view per workgroup
__global__ void __launch_bounds__(SIMP_THREADS)
simplify_clean_kernel(const MeshViewDev *__restrict__ cams, const SimpView *__restrict__ views)
{
#pragma clang fp contract(off)
    SimpView const V = views[blockIdx.x];
    MeshViewDev const &C = cams[blockIdx.x];
    int const tid = threadIdx.x;
    int const T = V.result[R_NTRI], nv0 = V.result[R_NVERT] - 4;
    Quads q{ V.next, V.datum, V.verts };
    // S9: the triangles in id order; the ones at a corner go, ids shift by 4
    for (int t = tid; t < T; t += SIMP_THREADS) {
        uint32_t e = V.tri_start[t];
        bool keep = true;
        for (int k = 0; k < 3; ++k) {
            uint32_t const id = q.orig(e);
            V.f2[3 * (size_t)t + k] = id;
            keep = keep && id >= 4;
            e = q.lprev(e);
        }
        V.sa[t] = keep ? 1u : 0u;
        V.sb[t] = keep ? 1u : 0u;
    }
    for (int i = tid; i < nv0; i += SIMP_THREADS) {
        const double *v = V.verts + 3 * (size_t)(i + 4);
        float const x = (float)v[0], y = (float)v[1], z = (float)v[2];
        const uint8_t *px = V.image + ((size_t)(int)y * V.w + (int)x) * V.channels;
        V.rgb0[3 * (size_t)i] = px[0];
        V.rgb0[3 * (size_t)i + 1] = V.channels >= 3 ? px[1] : px[0];
        V.rgb0[3 * (size_t)i + 2] = V.channels >= 3 ? px[2] : px[0];
        world_point(C, (int)x, (int)y, z, V.pos0 + 3 * (size_t)i);
    }
    __threadfence_block();
    __syncthreads();
    int const F1 = (int)block_scan_u32(V.sb, T);
    for (int t = tid; t < T; t += SIMP_THREADS)
        if (V.sa[t])
            for (int k = 0; k < 3; ++k)
                V.f1[3 * (size_t)V.sb[t] + k] = V.f2[3 * (size_t)t + k] - 4;
    __threadfence_block();
    __syncthreads();
    // S10: face k against triangle k's zero count, and the edge ratio
    for (int k = tid; k < F1; k += SIMP_THREADS) {
        uint32_t const a = V.f1[3 * (size_t)k], b = V.f1[3 * (size_t)k + 1],
            c = V.f1[3 * (size_t)k + 2];
        float const e1 = edge_length(V.pos0, a, b), e2 = edge_length(V.pos0, a, c),
            e3 = edge_length(V.pos0, b, c);
        float const lo = fminf(e1, fminf(e2, e3)), hi = fmaxf(e1, fmaxf(e2, e3));
        bool const bad = V.tri_nzero[k] > 4 || (double)(lo / hi) < 0.1;
        V.sa[k] = bad ? 1u : 0u;
        V.sb[k] = bad ? 1u : 0u;
    }
    __threadfence_block();
    __syncthreads();
    // S11: slot i < n_valid keeps a valid face; the j-th invalid slot below
    // n_valid receives the j-th valid face from the end
    int const n_valid = F1 - (int)block_scan_u32(V.sb, F1);
    for (int k = tid; k < F1; k += SIMP_THREADS) {
        if (k >= n_valid)
            continue;
        if (V.sa[k])
            V.changed[V.sb[k]] = (uint32_t)k;
        else
            for (int r = 0; r < 3; ++r)
                V.f2[3 * (size_t)k + r] = V.f1[3 * (size_t)k + r];
    }
    __threadfence_block();
    __syncthreads();
    for (int k = n_valid + tid; k < F1; k += SIMP_THREADS) {
        if (V.sa[k])
            continue;
        int const valid_before = k - (int)V.sb[k];
        uint32_t const dst = V.changed[n_valid - valid_before - 1];
        for (int r = 0; r < 3; ++r)
            V.f2[3 * (size_t)dst + r] = V.f1[3 * (size_t)k + r];
    }
    // S12
    for (int i = tid; i < nv0; i += SIMP_THREADS)
        V.vflag[i] = 0;
    __threadfence_block();
    __syncthreads();
    for (int k = tid; k < 3 * n_valid; k += SIMP_THREADS)
        V.vflag[V.f2[k]] = 1;
    __threadfence_block();
    __syncthreads();
    for (int i = tid; i < nv0; i += SIMP_THREADS)
        V.vmap[i] = V.vflag[i];
    __threadfence_block();
    __syncthreads();
    int const n_out = (int)block_scan_u32(V.vmap, nv0);
    for (int i = tid; i < nv0; i += SIMP_THREADS) {
        if (!V.vflag[i])
            continue;
        size_t const j = V.vmap[i];
        for (int r = 0; r < 3; ++r) {
            V.pos[3 * j + r] = V.pos0[3 * (size_t)i + r];
            V.rgb[3 * j + r] = V.rgb0[3 * (size_t)i + r];
        }
    }
    for (int k = tid; k < 3 * n_valid; k += SIMP_THREADS)
        V.f2[k] = V.vmap[V.f2[k]];
    if (tid == 0) {
        V.result[R_OUT_V] = n_out;
        V.result[R_OUT_F] = n_valid;
    }
}

struct SimpOut {
    float *xyz, *nrm, *conf, *val;
    uint8_t *rgb;
    uint32_t *faces;
    int mesh, clip;
    float3 lo, hi;
};

// the edge of face f that follows vertex v in it
__device__ __forceinline__ void
face_edge(const uint32_t *faces, uint32_t f, uint32_t v, uint32_t &v1, uint32_t &v2)
{
    const uint32_t *t = faces + 3 * (size_t)f;
    int const j = t[0] == v ? 0 : (t[1] == v ? 1 : 2);
    v1 = t[(j + 1) % 3];
    v2 = t[(j + 2) % 3];
}

// S13 for one view per workgroup: P8-P12 (or M3-M5) on the irregular mesh
__global__ void __launch_bounds__(SIMP_THREADS)
simplify_attrs_kernel(const MeshViewDev *__restrict__ cams, const SimpView *__restrict__ views,
    SimpOut O)
{
#pragma clang fp contract(off)
    SimpView const V = views[blockIdx.x];
    MeshViewDev const &C = cams[blockIdx.x];
    int const tid = threadIdx.x;
    int const nv = V.result[R_OUT_V], nf = V.result[R_OUT_F];
    // the faces of every vertex in face-id order: count, scan, fill, sort
    for (int i = tid; i <= nv; i += SIMP_THREADS)
        V.adj_cnt[i] = 0;
    __threadfence_block();
    __syncthreads();
    for (int k = tid; k < 3 * nf; k += SIMP_THREADS)
        atomicAdd(&V.adj_cnt[V.f2[k]], 1u);
    __threadfence_block();
    __syncthreads();
    for (int i = tid; i <= nv; i += SIMP_THREADS) {
        V.adj_off[i] = i < nv ? V.adj_cnt[i] : 0u;
        V.vmap[i] = 0;
    }
    __threadfence_block();
    __syncthreads();
    (void)block_scan_u32(V.adj_off, nv + 1);
    for (int k = tid; k < 3 * nf; k += SIMP_THREADS) {
        uint32_t const v = V.f2[k];
        V.adj[V.adj_off[v] + atomicAdd(&V.vmap[v], 1u)] = (uint32_t)(k / 3);
    }
    __threadfence_block();
    __syncthreads();
    for (int v = tid; v < nv; v += SIMP_THREADS) {
        uint32_t *L = V.adj + V.adj_off[v];
        int const deg = (int)V.adj_cnt[v];
        for (int i = 1; i < deg; ++i) {
            uint32_t const x = L[i];
            int j = i;
            for (; j > 0 && L[j - 1] > x; --j)
                L[j] = L[j - 1];
            L[j] = x;
        }
        // MeshInfo::update_vertex: chain the edges front and back (P8)
        uint32_t *R = V.nbr + 2 * (size_t)V.adj_off[v];
        int head = deg - 1, tail = deg;
        uint32_t front, back;
        face_edge(V.f2, L[0], (uint32_t)v, front, back);
        R[head] = front;
        int left = deg - 1;
        uint32_t const used = 0x80000000u;
        L[0] |= used;
        while (left > 0) {
            bool appended = false;
            for (int k = 1; k < deg; ++k) {
                if (L[k] & used)
                    continue;
                uint32_t a, b;
                face_edge(V.f2, L[k], (uint32_t)v, a, b);
                if (a == back) {
                    R[tail++] = a;
                    back = b;
                } else if (b == front) {
                    R[--head] = a;
                    front = a;
                } else
                    continue;
                L[k] |= used;
                --left;
                appended = true;
                break;
            }
            if (!appended)
                break;
        }
        for (int k = 0; k < deg; ++k)
            L[k] &= ~used;
        bool border = false;
        if (left > 0) {
            // complex: the other vertices of all faces, sorted, unique
            int n = 0;
            for (int k = 0; k < deg; ++k) {
                uint32_t a, b;
                face_edge(V.f2, L[k], (uint32_t)v, a, b);
                R[n++] = a;
                R[n++] = b;
            }
            for (int i = 1; i < n; ++i) {
                uint32_t const x = R[i];
                int j = i;
                for (; j > 0 && R[j - 1] > x; --j)
                    R[j] = R[j - 1];
                R[j] = x;
            }
            int u = 0;
            for (int i = 0; i < n; ++i)
                if (u == 0 || R[u - 1] != R[i])
                    R[u++] = R[i];
            head = 0;
            tail = u;
        } else if (front != back) {
            border = true;
            R[tail++] = back;
        }
        V.nbr_at[v] = (uint32_t)head;
        V.nbr_cnt[v] = (uint32_t)(tail - head);
        V.dist[0][v] = border ? 0 : 4;
    }
    __threadfence_block();
    __syncthreads();
    // P10: three relaxations of the hop distance to the nearest border vertex
    for (int round = 0; round < 3; ++round) {
        int const src = round & 1;
        for (int v = tid; v < nv; v += SIMP_THREADS) {
            const uint32_t *R = V.nbr + 2 * (size_t)V.adj_off[v] + V.nbr_at[v];
            int d = V.dist[src][v];
            for (uint32_t k = 0; k < V.nbr_cnt[v]; ++k) {
                int const dn = V.dist[src][R[k]] + 1;
                d = dn < d ? dn : d;
            }
            V.dist[src ^ 1][v] = (uint8_t)d;
        }
        __threadfence_block();
        __syncthreads();
    }
    for (int k = tid; k < 3 * nf; k += SIMP_THREADS)
        if (O.faces != nullptr)
            O.faces[3 * V.out_f + k] = V.f2[k] + (uint32_t)V.out_v;
    for (int v = tid; v < nv; v += SIMP_THREADS) {
        size_t const id = V.out_v + v;
        const float *pos = V.pos + 3 * (size_t)v;
        for (int r = 0; r < 3; ++r) {
            O.xyz[3 * id + r] = pos[r];
            O.rgb[3 * id + r] = V.rgb[3 * (size_t)v + r];
        }
        int const d = V.dist[1][v];
        O.conf[id] = d >= 4 ? 1.0f : (float)d / 4.0f;
        float n[3] = { 0.0f, 0.0f, 0.0f };
        if (O.mesh) {
            // M3-M5 as a gather over the vertex's faces in face-id order
            const uint32_t *L = V.adj + V.adj_off[v];
            for (uint32_t k = 0; k < V.adj_cnt[v]; ++k) {
                const uint32_t *t = V.f2 + 3 * (size_t)L[k];
                float q[3][3];
                bool keep = true;
                int k_me = 0;
                for (int c = 0; c < 3; ++c) {
                    for (int r = 0; r < 3; ++r)
                        q[c][r] = V.pos[3 * (size_t)t[c] + r];
                    if (O.clip && outside_aabb(q[c], O.lo, O.hi))
                        keep = false;
                    if (t[c] == (uint32_t)v)
                        k_me = c;
                }
                float fn[3], weight;
                if (!keep || !face_term(q, k_me, fn, &weight))
                    continue;
                for (int r = 0; r < 3; ++r)
                    n[r] += fn[r] * weight;
            }
            float const len = sqrtf(dot3(n, n));
            if (len > 0.0f)
                for (int r = 0; r < 3; ++r)
                    n[r] = n[r] / len;
        } else {
            // P12: the normal map at the vertex's projection; P11: the scale value
            float const u = dot3(C.KR + 0, pos) - C.t[0];
            float const vv = dot3(C.KR + 3, pos) - C.t[1];
            float const ww = dot3(C.KR + 6, pos) - C.t[2];
            float const qx = u / ww, qy = vv / ww;
            if (qx > -1.0f && qx < (float)V.w && qy > -1.0f && qy < (float)V.h) {
                size_t const p = (size_t)(int)qy * V.w + (int)qx;
                for (int r = 0; r < 3; ++r)
                    n[r] = C.normals[3 * p + r];
            }
            const uint32_t *R = V.nbr + 2 * (size_t)V.adj_off[v] + V.nbr_at[v];
            uint32_t const cnt = V.nbr_cnt[v];
            float s = 0.0f;
            for (uint32_t k = 0; k < cnt; ++k)
                s += edge_length(V.pos, (uint32_t)v, R[k]);
            s /= (float)cnt;
            s *= 2.0f;
            O.val[id] = s;
        }
        for (int r = 0; r < 3; ++r)
            O.nrm[3 * id + r] = n[r];
    }
}

// ----------------------------------------------- AABB clip: the face passes
// (the vertex passes are export_common.hip's launch_aabb_clip)
__global__ void __launch_bounds__(256)
simplify_face_keep_kernel(const uint32_t *__restrict__ faces, size_t m,
    const float *__restrict__ xyz, float3 lo, float3 hi, unsigned long long *__restrict__ keep)
{
    size_t const f = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= m)
        return;
    bool k = true;
    for (int c = 0; c < 3; ++c)
        k = k && !outside_aabb(xyz + 3 * (size_t)faces[3 * f + c], lo, hi);
    keep[f] = k ? 1ull : 0ull;
}

__global__ void __launch_bounds__(256)
simplify_face_scatter_kernel(const uint32_t *__restrict__ faces, size_t m,
    const float *__restrict__ xyz, float3 lo, float3 hi,
    const unsigned long long *__restrict__ at, const unsigned long long *__restrict__ vmap,
    uint32_t *__restrict__ out)
{
    size_t const f = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= m)
        return;
    for (int c = 0; c < 3; ++c)
        if (outside_aabb(xyz + 3 * (size_t)faces[3 * f + c], lo, hi))
            return;
    for (int c = 0; c < 3; ++c)
        out[3 * (size_t)at[f] + c] = (uint32_t)vmap[faces[3 * f + c]];
}

} // namespace smvs_hip

using namespace smvs_hip;

namespace {

// the arena of one view, carved from the slab
struct ArenaPlan {
    size_t at[32];
};

void
plan_arena(Carver &carve, SimpView &V, ArenaPlan &P)
{
    size_t const nv = (size_t)V.max_verts, nt = (size_t)V.max_tris, ne = (size_t)V.max_edges;
    int k = 0;
    P.at[k++] = carve(24 * nv);         // verts
    P.at[k++] = carve(16 * ne);         // next
    P.at[k++] = carve(16 * ne);         // datum
    P.at[k++] = carve(4 * nt);          // tri_start
    P.at[k++] = carve(8 * nt);          // tri_key
    P.at[k++] = carve(4 * nt);          // tri_stamp
    P.at[k++] = carve(12 * nt);         // tri_cand
    P.at[k++] = carve(4 * nt);          // tri_nzero
    P.at[k++] = carve(4 * nt);          // changed
    P.at[k++] = carve(4 * R_NUM);       // result
    P.at[k++] = carve(8 * 4);           // clocks
    P.at[k++] = carve(12 * nv);         // pos0
    P.at[k++] = carve(12 * nv);         // pos
    P.at[k++] = carve(3 * nv);          // rgb0
    P.at[k++] = carve(3 * nv);          // rgb
    P.at[k++] = carve(12 * nt);         // f1
    P.at[k++] = carve(12 * nt);         // f2
    P.at[k++] = carve(4 * (nt + 1));    // sa
    P.at[k++] = carve(4 * (nt + 1));    // sb
    P.at[k++] = carve(4 * (nv + 1));    // vmap
    P.at[k++] = carve(4 * (nv + 1));    // adj_off
    P.at[k++] = carve(4 * (nv + 1));    // adj_cnt
    P.at[k++] = carve(12 * nt);         // adj
    P.at[k++] = carve(24 * nt);         // nbr
    P.at[k++] = carve(4 * nv);          // nbr_at
    P.at[k++] = carve(4 * nv);          // nbr_cnt
    P.at[k++] = carve(nv);              // dist[0]
    P.at[k++] = carve(nv);              // dist[1]
    P.at[k++] = carve(nv);              // vflag
}

void
bind_arena(char *slab, ArenaPlan const &P, SimpView &V)
{
    int k = 0;
    auto at = [&](auto *&p) {
        p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(slab + P.at[k++]);
    };
    at(V.verts); at(V.next); at(V.datum); at(V.tri_start); at(V.tri_key); at(V.tri_stamp);
    at(V.tri_cand); at(V.tri_nzero); at(V.changed); at(V.result); at(V.clocks); at(V.pos0);
    at(V.pos); at(V.rgb0); at(V.rgb); at(V.f1); at(V.f2); at(V.sa); at(V.sb); at(V.vmap);
    at(V.adj_off); at(V.adj_cnt); at(V.adj); at(V.nbr); at(V.nbr_at); at(V.nbr_cnt);
    at(V.dist[0]); at(V.dist[1]); at(V.vflag);
}

// S1 and the sizes that follow from it
int
size_view(int width, int height, int max_vertices, double max_error, SimpView &V)
{
    SMVS_REQUIRE(width >= 2 && height >= 2, "a depth map needs at least 2 x 2 pixels");
    SMVS_REQUIRE(width <= 4096 && height <= 4096, "a depth map may be at most 4096 x 4096");
    SMVS_REQUIRE(max_vertices >= -1 && max_vertices <= (1 << 24), "bad max_vertices");
    SMVS_REQUIRE(max_error == -1.0 || (max_error >= 0.0 && std::isfinite(max_error)),
        "max_error must be -1 or finite and >= 0");
    size_t const npix = (size_t)width * height;
    V.w = width;
    V.h = height;
    V.budget = max_vertices < 0 ? (int)(npix / 40) : max_vertices;
    V.max_error = max_error;
    // no more distinct points than pixels can be inserted (S5 ends the rest)
    size_t const inserts = std::min((size_t)V.budget, npix) + 1;
    V.max_verts = (int)(inserts + 4);
    V.max_tris = (int)(2 * inserts + 2);
    V.max_edges = (int)(4 * inserts + 5);
    return SMVS_OK;
}

int
check_depths(const float *depth, size_t n)
{
    for (size_t i = 0; i < n; ++i)
        SMVS_REQUIRE(std::isfinite(depth[i]) && depth[i] >= 0.0f,
            "depths must be finite and >= 0");
    return SMVS_OK;
}

int
greedy_status(int status, int view)
{
    if (status == SIMP_OK)
        return SMVS_OK;
    set_error("smvs_simplify: view %d ended with status %d (%s)", view, status,
        status == SIMP_WALK_CAP ? "a walk over the subdivision hit its cap"
        : status == SIMP_ARENA ? "the view's arena is full" : "a triangle has too many rows");
    return SMVS_ERR_STATE;
}

} // namespace

extern "C" int
smvs_simplify_triangulate(int device, const float *depth, int width, int height,
    int max_vertices, double max_error, int64_t *iterations, int64_t *n_vertices,
    double *vertices, int64_t *n_triangles, uint32_t *triangles, int32_t *num_zero_depths,
    uint64_t *clocks4)
{
    SMVS_REQUIRE(depth != nullptr, "no depth map");
    SimpView V = {};
    int rc;
    if ((rc = size_view(width, height, max_vertices, max_error, V))
        || (rc = check_depths(depth, (size_t)width * height)))
        return rc;
    WorkspaceLease lease(device);
    if (lease.w == nullptr)
        return SMVS_ERR_HIP;
    Workspace &ws = *lease.w;
    Carver carve;
    size_t const npix = (size_t)width * height;
    size_t const dm_at = carve(4 * npix), table_at = carve(sizeof(SimpView));
    ArenaPlan plan;
    plan_arena(carve, V, plan);
    char *slab = nullptr;
    if ((rc = ws.ensure(0, carve.total, &slab)) != SMVS_OK)
        return rc;
    bind_arena(slab, plan, V);
    V.dm = reinterpret_cast<float *>(slab + dm_at);
    V.channels = 1;
    SimpView *d_table = reinterpret_cast<SimpView *>(slab + table_at);
    if ((rc = ws.upload(const_cast<float *>(V.dm), depth, 4 * npix))
        || (rc = ws.upload(d_table, &V, sizeof(V))))
        return rc;
    if (clocks4 != nullptr)
        hipLaunchKernelGGL(simplify_greedy_kernel<true>, dim3(1), dim3(SIMP_THREADS), 0,
            ws.stream, d_table);
    else
        hipLaunchKernelGGL(simplify_greedy_kernel<false>, dim3(1), dim3(SIMP_THREADS), 0,
            ws.stream, d_table);
    SMVS_HIP_CHECK(hipGetLastError());
    int result[R_NUM];
    if ((rc = ws.download(result, V.result, sizeof(result)))
        || (rc = greedy_status(result[R_STATUS], 0)))
        return rc;
    size_t const nv = (size_t)result[R_NVERT], nt = (size_t)result[R_NTRI];
    if (iterations != nullptr)
        *iterations = result[R_ITER];
    if (n_vertices != nullptr)
        *n_vertices = (int64_t)nv;
    if (n_triangles != nullptr)
        *n_triangles = (int64_t)nt;
    if (clocks4 != nullptr && (rc = ws.download(clocks4, V.clocks, 32)))
        return rc;
    if (vertices != nullptr && (rc = ws.download(vertices, V.verts, 24 * nv)))
        return rc;
    if (num_zero_depths != nullptr && (rc = ws.download(num_zero_depths, V.tri_nzero, 4 * nt)))
        return rc;
    if (triangles != nullptr) {
        // a triangle's vertices: start.orig, then l_prev twice (S4)
        std::vector<uint32_t> next(4 * (size_t)V.max_edges), datum(next.size()), start(nt);
        if ((rc = ws.download(next.data(), V.next, 4 * next.size()))
            || (rc = ws.download(datum.data(), V.datum, 4 * datum.size()))
            || (rc = ws.download(start.data(), V.tri_start, 4 * nt)))
            return rc;
        for (size_t t = 0; t < nt; ++t) {
            uint32_t e = start[t];
            for (int k = 0; k < 3; ++k) {
                triangles[3 * t + k] = datum[e];
                uint32_t const n = next[e];
                e = (n & ~3u) | ((n + 2) & 3u);
            }
        }
    }
    return SMVS_OK;
}

extern "C" int
smvs_simplified_generate(int device, const smvs_point_view *views, int n_views,
    const smvs_simplify_options *options, smvs_points **handle, int64_t *n_vertices,
    int64_t *n_faces)
{
    SMVS_REQUIRE(handle != nullptr, "no handle pointer");
    *handle = nullptr;
    smvs_simplify_options opt = { 1, 0, { 0, 0, 0 }, { 0, 0, 0 }, 0, -1, -1.0 };
    if (options != nullptr)
        opt = *options;
    SMVS_REQUIRE(views != nullptr && n_views >= 1, "no views");
    SMVS_REQUIRE(n_views <= 4096, "too many views");
    std::vector<SimpView> stable(n_views);
    int rc;
    for (int i = 0; i < n_views; ++i) {
        smvs_point_view const &in = views[i];
        SMVS_REQUIRE(in.depth != nullptr && in.normals != nullptr && in.image != nullptr
            && in.channels >= 1 && in.channels <= 4 && in.flen > 0.0f, "bad view");
        if ((rc = size_view(in.width, in.height, opt.max_vertices, opt.max_error, stable[i]))
            || (rc = check_depths(in.depth, (size_t)in.width * in.height)))
            return rc;
        stable[i].channels = in.channels;
    }
    bool const mesh = opt.create_triangle_mesh != 0, clip = opt.use_aabb != 0;
    bool const cut = opt.cut_surfaces != 0;

    WorkspaceLease lease(device);
    if (lease.w == nullptr)
        return SMVS_ERR_HIP;
    Workspace &ws = *lease.w;
    Carver carve;
    ViewSlab s;
    carve_views(views, n_views, true, carve, s);
    std::vector<ArenaPlan> plans(n_views);
    for (int i = 0; i < n_views; ++i)
        plan_arena(carve, stable[i], plans[i]);
    size_t const table_at = carve(sizeof(SimpView) * n_views);
    char *slab = nullptr;
    if ((rc = ws.ensure(0, carve.total, &slab)) != SMVS_OK)
        return rc;
    hipStream_t const stream = ws.stream;
    if ((rc = upload_and_prepare(ws, slab, views, n_views, cut, true, s)))
        return rc;
    MeshViewDev *const d_cams = s.d_table;
    for (int i = 0; i < n_views; ++i) {
        SimpView &V = stable[i];
        bind_arena(slab, plans[i], V);
        // generate_mesh triangulates the cut maps, or the depth maps (:211-213)
        V.dm = cut ? s.table[i].cut : s.table[i].depth_ray;
        V.image = s.images[i];
    }
    SimpView *d_table = reinterpret_cast<SimpView *>(slab + table_at);
    if ((rc = ws.upload(d_table, stable.data(), sizeof(SimpView) * n_views)))
        return rc;
    hipLaunchKernelGGL(simplify_greedy_kernel<false>, dim3(n_views), dim3(SIMP_THREADS), 0,
        stream, d_table);
    hipLaunchKernelGGL(simplify_clean_kernel, dim3(n_views), dim3(SIMP_THREADS), 0, stream,
        d_cams, d_table);
    SMVS_HIP_CHECK(hipGetLastError());
    // the views' sizes -> their offsets in the merged mesh (M1, view-list order)
    size_t n_vert = 0, n_face = 0;
    for (int i = 0; i < n_views; ++i) {
        int result[R_NUM];
        if ((rc = ws.download(result, stable[i].result, sizeof(result)))
            || (rc = greedy_status(result[R_STATUS], i)))
            return rc;
        stable[i].out_v = n_vert;
        stable[i].out_f = n_face;
        n_vert += (size_t)result[R_OUT_V];
        n_face += (size_t)result[R_OUT_F];
    }
    SMVS_REQUIRE(n_vert < ((size_t)1 << 31), "too many vertices");
    if ((rc = ws.upload(d_table, stable.data(), sizeof(SimpView) * n_views)))
        return rc;
    bool const faces_out = mesh || !clip;
    // the merged mesh, and the stage of the clip
    Carver oc;
    size_t out_at[2][6];
    size_t const nv1 = n_vert + 1, nf1 = n_face + 1;
    for (int k = 0; k < (clip ? 2 : 1); ++k) {
        out_at[k][0] = oc(12 * nv1);
        out_at[k][1] = oc(12 * nv1);
        out_at[k][2] = oc(3 * nv1);
        out_at[k][3] = oc(4 * nv1);
        out_at[k][4] = oc(4 * nv1);
        out_at[k][5] = oc(12 * nf1);
    }
    size_t const n_big = std::max(nv1, nf1), n_tiles = (n_big + SCAN_TILE - 1) / SCAN_TILE;
    size_t const vscan_at = oc(8 * nv1), fscan_at = oc(8 * nf1),
        tiles_at = oc(8 * (n_tiles + 1)), ftiles_at = oc(8 * (n_tiles + 1));
    char *outs = nullptr;
    if ((rc = ws.ensure(1, oc.total, &outs)) != SMVS_OK)
        return rc;
    auto outputs = [&](SimpOut &o, int k) {
        o.xyz = reinterpret_cast<float *>(outs + out_at[k][0]);
        o.nrm = reinterpret_cast<float *>(outs + out_at[k][1]);
        o.rgb = reinterpret_cast<uint8_t *>(outs + out_at[k][2]);
        o.conf = reinterpret_cast<float *>(outs + out_at[k][3]);
        o.val = mesh ? nullptr : reinterpret_cast<float *>(outs + out_at[k][4]);
        o.faces = reinterpret_cast<uint32_t *>(outs + out_at[k][5]);
    };
    SimpOut A = {};
    outputs(A, 0);
    A.mesh = mesh ? 1 : 0;
    A.clip = clip ? 1 : 0;
    A.lo = make_float3(opt.aabb_min[0], opt.aabb_min[1], opt.aabb_min[2]);
    A.hi = make_float3(opt.aabb_max[0], opt.aabb_max[1], opt.aabb_max[2]);
    hipLaunchKernelGGL(simplify_attrs_kernel, dim3(n_views), dim3(SIMP_THREADS), 0, stream,
        d_cams, d_table, A);
    SMVS_HIP_CHECK(hipGetLastError());
    SimpOut O = A;
    if (clip && n_vert > 0) {
        unsigned long long *const vscan = reinterpret_cast<unsigned long long *>(outs + vscan_at);
        unsigned long long *const fscan = reinterpret_cast<unsigned long long *>(outs + fscan_at);
        unsigned long long *const tiles = reinterpret_cast<unsigned long long *>(outs + tiles_at);
        unsigned long long *const ftiles = reinterpret_cast<unsigned long long *>(outs + ftiles_at);
        outputs(O, 1);
        if ((rc = launch_aabb_clip(stream, n_vert, A.lo, A.hi, vertex_attrs(A), vertex_attrs(O),
                vscan, tiles)))
            return rc;
        unsigned long long sum = 0;
        if (mesh && n_face > 0) {
            unsigned const fblocks = (unsigned)((n_face + 255) / 256);
            hipLaunchKernelGGL(simplify_face_keep_kernel, dim3(fblocks), dim3(256), 0, stream,
                A.faces, n_face, A.xyz, A.lo, A.hi, fscan);
            SMVS_HIP_CHECK(hipGetLastError());
            if ((rc = exclusive_scan(stream, fscan, n_face, ftiles)))
                return rc;
            hipLaunchKernelGGL(simplify_face_scatter_kernel, dim3(fblocks), dim3(256), 0, stream,
                A.faces, n_face, A.xyz, A.lo, A.hi, fscan, vscan, O.faces);
            SMVS_HIP_CHECK(hipGetLastError());
            if ((rc = ws.download(&sum, scan_total(ftiles, n_face), sizeof(sum))))
                return rc;
            n_face = (size_t)sum;
        }
        if ((rc = ws.download(&sum, scan_total(tiles, n_vert), sizeof(sum))))
            return rc;
        n_vert = (size_t)sum;
    }
    for (int i = 0; i < n_views; ++i)
        if (views[i].cut_depth != nullptr
            && (rc = ws.download(views[i].cut_depth, stable[i].dm,
                    4 * (size_t)views[i].width * views[i].height)))
            return rc;
    if ((rc = fill_points(ws, mesh, false, n_vert, n_face, vertex_attrs(O),
            faces_out ? O.faces : nullptr, nullptr, handle)))
        return rc;
    if (n_vertices != nullptr)
        *n_vertices = (*handle)->n_points;
    if (n_faces != nullptr)
        *n_faces = (*handle)->n_faces;
    return SMVS_OK;
}
