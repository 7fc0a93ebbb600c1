// Serial CPU restatement of smvsrecon --simplify for one view (rows S1-S13 of
// DESIGN.md section 9.7): the greedy insertion of
// DepthTriangulator::approximate_triangulation over an incremental Delaunay
// triangulation on quad-edges, its clean-up, and after it the per-view export
// of tests/points_reference.cc (MeshInfo, confidences, scale value, normal
// lookup) on the irregular mesh.  The heap is a real std::multimap and the
// changed set a real std::set, so that S6's ordering is the library's.  Test
// infrastructure only: compiled by tests/simplify_ref.py with
// g++ -O2 -ffp-contract=off and loaded through ctypes; it shares no source
// with the HIP kernels.
#include "points_reference.cc"

#include <cfloat>
#include <functional>
#include <map>
#include <set>

namespace {

struct P2 {
    double x, y;
};

struct P3 {
    double x, y, z;
};

// ------------------------------------------------------------ S4: predicates
double area2(P2 a, P2 b, P2 c)
{
    return (b.x - a.x) * (c.y - a.y) - (b.y - a.y) * (c.x - a.x);
}

double sqn(P2 a)
{
    double s = 0.0;
    s += a.x * a.x;
    s += a.y * a.y;
    return s;
}

bool in_circle(P2 a, P2 b, P2 c, P2 p)
{
    return (sqn(a) * area2(b, c, p) - sqn(b) * area2(a, c, p) + sqn(c) * area2(a, b, p)
        - sqn(p) * area2(a, b, c)) > 0;
}

bool right_of(P2 p, P2 orig, P2 dest)
{
    return area2(p, dest, orig) > 0;
}

double dist2d(P2 a, P2 b)
{
    return std::sqrt(sqn(P2{ a.x - b.x, a.y - b.y }));
}

bool on_edge(P2 p, P2 orig, P2 dest)
{
    double const eps = 1e-5;
    double const t1 = dist2d(p, orig), t2 = dist2d(p, dest);
    if (t1 < eps || t2 < eps)
        return true;
    double const t3 = dist2d(orig, dest);
    if (t1 > t3 || t2 > t3)
        return false;
    double d = ((dest.y - orig.y) * p.x) - ((dest.x - orig.x) * p.y) + dest.x * orig.y
        - dest.y * orig.x;
    d /= t3;
    return std::fabs(d) < eps;
}

// ------------------------------------------------------- S4: the subdivision
// Quarter-edges are numbered 4 q + r (q the quad-edge, r its rotation); each
// carries the next quarter-edge around its origin and one datum: a vertex on
// the primal quarters (r even), a face on the dual ones.
struct Subdivision {
    std::vector<uint32_t> next, datum;
    std::vector<P3> verts;
    std::vector<uint32_t> tri_start;
    std::set<std::size_t> changed;

    static uint32_t rot(uint32_t e, int k) { return (e & ~3u) | ((e + k) & 3u); }
    static uint32_t inv(uint32_t e) { return rot(e, 2); }
    static uint32_t dual(uint32_t e) { return rot(e, 1); }
    static uint32_t idual(uint32_t e) { return rot(e, 3); }
    uint32_t onext(uint32_t e) const { return next[e]; }
    uint32_t oprev(uint32_t e) const { return dual(next[dual(e)]); }
    uint32_t dprev(uint32_t e) const { return idual(next[idual(e)]); }
    uint32_t lnext(uint32_t e) const { return dual(next[idual(e)]); }
    uint32_t lprev(uint32_t e) const { return inv(next[e]); }
    uint32_t &orig(uint32_t e) { return datum[e]; }
    uint32_t &dest(uint32_t e) { return datum[inv(e)]; }
    uint32_t &left(uint32_t e) { return datum[dual(e)]; }
    uint32_t &right(uint32_t e) { return datum[idual(e)]; }
    P2 at(uint32_t v) const { return P2{ verts[v].x, verts[v].y }; }

    uint32_t make_edge()
    {
        uint32_t const e = (uint32_t)next.size();
        next.push_back(e);
        next.push_back(e + 3);
        next.push_back(e + 2);
        next.push_back(e + 1);
        datum.resize(datum.size() + 4, 0u);
        return e;
    }

    void splice(uint32_t a, uint32_t b)
    {
        uint32_t const alpha = dual(next[a]), beta = dual(next[b]);
        uint32_t const an = next[a], bn = next[b], aln = next[alpha], ben = next[beta];
        next[a] = bn;
        next[b] = an;
        next[alpha] = ben;
        next[beta] = aln;
    }

    void set_ends(uint32_t e, uint32_t o, uint32_t d)
    {
        orig(e) = o;
        dest(e) = d;
    }

    uint32_t connect(uint32_t a, uint32_t b)
    {
        uint32_t const e = make_edge();
        splice(e, lnext(a));
        splice(inv(e), b);
        set_ends(e, dest(a), orig(b));
        return e;
    }

    void unlink(uint32_t e)
    {
        splice(e, oprev(e));
        splice(inv(e), oprev(inv(e)));
    }

    void flip(uint32_t e)
    {
        uint32_t const a = oprev(e), b = oprev(inv(e));
        splice(e, a);
        splice(inv(e), b);
        splice(e, lnext(a));
        splice(inv(e), lnext(b));
        set_ends(e, dest(a), dest(b));
        left(lnext(e)) = left(e);
        left(lprev(e)) = left(e);
        uint32_t const dn = inv(next[inv(e)]);
        left(dn) = right(e);
        left(oprev(e)) = right(e);
        tri_start[left(e)] = e;
        tri_start[right(e)] = inv(e);
        changed.insert(left(e));
        changed.insert(right(e));
    }

    // the bounding quad: triangle 0 = (p0, p1, p2), triangle 1 = (p1, p3, p2)
    void initialize(P3 p0, P3 p1, P3 p2, P3 p3)
    {
        verts = { p0, p1, p2, p3 };
        uint32_t const e1 = make_edge();
        set_ends(e1, 0, 1);
        uint32_t const e2 = make_edge();
        splice(inv(e1), e2);
        set_ends(e2, 1, 2);
        uint32_t const e3 = make_edge();
        splice(inv(e2), e3);
        set_ends(e3, 2, 0);
        splice(inv(e3), e1);
        tri_start.push_back(e1);
        left(e1) = left(e2) = left(e3) = 0;
        uint32_t const e4 = make_edge();
        splice(inv(e1), e4);
        set_ends(e4, 1, 3);
        uint32_t const e5 = make_edge();
        splice(inv(e4), e5);
        set_ends(e5, 3, 2);
        splice(inv(e5), inv(e2));
        tri_start.push_back(e4);
        left(e4) = left(e5) = 1;
        left(lnext(e5)) = 1;
        right(inv(lnext(e5))) = 1;
    }

    uint32_t locate(P2 p, uint32_t e) const
    {
        Subdivision &s = const_cast<Subdivision &>(*this);
        for (;;) {
            P2 const o = at(s.orig(e)), d = at(s.dest(e));
            if ((p.x == o.x && p.y == o.y) || (p.x == d.x && p.y == d.y))
                return e;
            if (right_of(p, o, d)) {
                e = inv(e);
                continue;
            }
            uint32_t const n = onext(e);
            if (!right_of(p, at(s.orig(n)), at(s.dest(n)))) {
                e = n;
                continue;
            }
            uint32_t const q = dprev(e);
            if (!right_of(p, at(s.orig(q)), at(s.dest(q)))) {
                e = q;
                continue;
            }
            return e;
        }
    }

    void insert(P3 p3, std::size_t triangle)
    {
        changed.clear();
        P2 const p{ p3.x, p3.y };
        uint32_t e = locate(p, tri_start[triangle]);
        P2 const o = at(orig(e)), d = at(dest(e));
        if ((p.x == o.x && p.y == o.y) || (p.x == d.x && p.y == d.y))
            return;   // S5
        if (on_edge(p, o, d)) {
            e = oprev(e);
            unlink(onext(e));
        }
        uint32_t base = make_edge();
        verts.push_back(p3);
        uint32_t const pv = (uint32_t)verts.size() - 1;
        set_ends(base, orig(e), pv);
        right(base) = left(e);
        tri_start[left(e)] = e;
        changed.insert(left(e));
        splice(base, e);
        uint32_t const first = base;
        for (int i = 0; i < 2; ++i) {
            base = connect(e, inv(base));
            left(base) = left(e);
            e = oprev(base);
            tri_start.push_back(e);
            changed.insert(tri_start.size() - 1);
            left(e) = (uint32_t)tri_start.size() - 1;
            right(base) = left(e);
        }
        if (lnext(e) != first) {
            base = connect(e, inv(base));
            left(base) = left(e);
            e = oprev(base);
            tri_start[left(e)] = e;
            changed.insert(left(e));
            right(base) = left(e);
        }
        left(first) = left(e);
        for (;;) {
            uint32_t const t = oprev(e);
            if (right_of(at(dest(t)), at(orig(e)), at(dest(e)))
                && in_circle(at(orig(e)), at(dest(t)), at(dest(e)), p)) {
                flip(e);
                e = oprev(e);
            } else if (onext(e) == first)
                return;
            else
                e = lprev(onext(e));
        }
    }

    void triangle(std::size_t t, uint32_t *ids)
    {
        uint32_t e = tri_start[t];
        for (int k = 0; k < 3; ++k) {
            ids[k] = orig(e);
            e = lprev(e);
        }
    }
};

// ----------------------------------------------------------- S8: rasteriser
typedef std::vector<std::pair<int, int>> PixelList;

void pixels_bottom_flat(P2 a, P2 b, P2 c, PixelList &out, int variant)
{
    double const d1 = (c.x - a.x) / (c.y - a.y), d2 = (c.x - b.x) / (c.y - b.y);
    double x1 = c.x, x2 = c.x;
    int r = 0;
    for (int y = (int)c.y; y > b.y; y--) {
        for (int x = (int)std::ceil(std::min(x1, x2)); x <= (int)std::floor(std::max(x1, x2)); ++x)
            out.emplace_back(x, y);
        x1 -= d1;
        x2 -= d2;
        if (variant == V_S8_MULTIPLY) {
            ++r;
            x1 = c.x - r * d1;
            x2 = c.x - r * d2;
        }
    }
}

void pixels_top_flat(P2 a, P2 b, P2 c, PixelList &out, int variant)
{
    double const d1 = (a.x - c.x) / (a.y - c.y), d2 = (a.x - b.x) / (a.y - b.y);
    double x1 = a.x, x2 = a.x;
    int r = 0;
    for (int y = (int)a.y; y <= b.y; y++) {
        for (int x = (int)std::ceil(std::min(x1, x2)); x <= (int)std::floor(std::max(x1, x2)); ++x)
            out.emplace_back(x, y);
        x1 += d1;
        x2 += d2;
        if (variant == V_S8_MULTIPLY) {
            ++r;
            x1 = a.x + r * d1;
            x2 = a.x + r * d2;
        }
    }
}

void pixels_for_triangle(P2 a, P2 b, P2 c, PixelList &out, int variant = V_PINNED)
{
    P2 v[3] = { a, b, c };
    std::stable_sort(v, v + 3, [](P2 const &l, P2 const &r) { return l.y < r.y; });
    if (v[1].y == v[2].y)
        pixels_top_flat(v[0], v[1], v[2], out, variant);
    else if (v[0].y == v[1].y)
        pixels_bottom_flat(v[0], v[1], v[2], out, variant);
    else {
        P2 m{ v[0].x + ((v[1].y - v[0].y) / (v[2].y - v[0].y)) * (v[2].x - v[0].x), v[1].y };
        m.x = v[0].x < v[1].x ? std::ceil(m.x) : std::floor(m.x);
        pixels_top_flat(v[0], v[1], m, out, variant);
        pixels_bottom_flat(v[1], m, v[2], out, variant);
    }
}

// ------------------------------------------------------ S6 / S7: greedy loop
typedef std::multimap<double, std::size_t, std::greater<double>> Heap;

struct ScanTriangle {
    P3 v[3];
    P3 candidate{ 0, 0, 0 };
    int num_zero = 0;
    Heap::iterator at;
};

struct Greedy {
    int w, h;
    const float *dm;
    Subdivision sub;
    std::vector<ScanTriangle> tris;
    Heap heap;
    long long iterations = 0;
    int variant = V_PINNED;
    // what the loop met: iterations whose top key another triangle shares
    // (S6), scans in which a later pixel equals the best distance (S7), no-op
    // insertions (S5), the most rows a scanned triangle spans
    long long tied_tops = 0, tied_scans = 0, noop_insertions = 0, max_rows = 0;

    // S6: begin(), the earliest emplaced of the largest key
    Heap::iterator top()
    {
        if (variant == V_S6_LATEST)
            return std::prev(heap.upper_bound(heap.begin()->first));
        return heap.begin();
    }

    void load(std::size_t id)
    {
        uint32_t ids[3];
        sub.triangle(id, ids);
        for (int k = 0; k < 3; ++k)
            tris[id].v[k] = sub.verts[ids[k]];
    }

    void scan(std::size_t id)
    {
        ScanTriangle &t = tris[id];
        PixelList px;
        pixels_for_triangle(P2{ t.v[0].x, t.v[0].y }, P2{ t.v[1].x, t.v[1].y },
            P2{ t.v[2].x, t.v[2].y }, px, variant);
        if (!px.empty()) {
            auto const rows = std::minmax_element(px.begin(), px.end(),
                [](std::pair<int, int> const &l, std::pair<int, int> const &r) {
                    return l.second < r.second;
                });
            max_rows = std::max(max_rows, (long long)(rows.second->second - rows.first->second + 1));
        }
        // S7: the plane through the three vertices, unit normal
        double const ux = t.v[1].x - t.v[0].x, uy = t.v[1].y - t.v[0].y, uz = t.v[1].z - t.v[0].z;
        double const vx = t.v[2].x - t.v[0].x, vy = t.v[2].y - t.v[0].y, vz = t.v[2].z - t.v[0].z;
        double n[3] = { uy * vz - uz * vy, uz * vx - ux * vz, ux * vy - uy * vx };
        double len = 0.0;
        for (int k = 0; k < 3; ++k)
            len += n[k] * n[k];
        len = std::sqrt(len);
        for (int k = 0; k < 3; ++k)
            n[k] = n[k] / len;
        double dot = 0.0;
        dot += t.v[0].x * n[0];
        dot += t.v[0].y * n[1];
        dot += t.v[0].z * n[2];
        double const d = -dot;
        double best = 0;
        P3 cand{ 0.0, 0.0, 0.0 };
        t.num_zero = 0;
        bool tied = false;
        for (auto const &p : px) {
            if (p.first < 0 || p.first > w - 1 || p.second < 0 || p.second > h - 1)
                continue;
            float const depth = dm[(std::size_t)p.second * w + p.first];
            if (depth == 0) {
                t.num_zero += 1;
                continue;
            }
            double const dist = std::fabs(n[0] * p.first + n[1] * p.second + n[2] * depth + d);
            tied = tied || (dist == best && best > 0);
            if (variant == V_S7_GE ? dist >= best : dist > best) {
                best = dist;
                cand = P3{ (double)p.first, (double)p.second, (double)depth };
            }
        }
        t.candidate = cand;
        tied_scans += tied;
        heap.erase(t.at);
        t.at = heap.emplace(best, id);
    }

    void run(int max_vertices, double max_error)
    {
        std::size_t const npix = (std::size_t)w * h;
        if (max_vertices < 0)
            max_vertices = (int)(npix / 40);   // S1
        // S2
        float dm_max = dm[0];
        for (std::size_t i = 0; i < npix; ++i)
            dm_max = std::max(dm_max, dm[i]);
        float avg = 0, counter = 0;
        for (std::size_t i = 0; i < npix; ++i)
            if (dm[i] > 0) {
                avg += dm[i];
                counter += 1;
            }
        avg /= counter;
        if (max_error < 0.0)
            max_error = (dm_max - avg) * 1e-3;
        // S3
        auto corner = [&](int x, int y, int px, int py) {
            float const d = dm[(std::size_t)py * w + px];
            if (variant == V_S3_NO_FALLBACK)
                return P3{ (double)x, (double)y, (double)d };
            return P3{ (double)x, (double)y, d > 0 ? (double)d : (double)dm_max };
        };
        sub.initialize(corner(-1, -1, 0, 0), corner(w, -1, w - 1, 0), corner(-1, h, 0, h - 1),
            corner(w, h, w - 1, h - 1));
        for (std::size_t id = 0; id < 2; ++id) {
            tris.emplace_back();
            load(id);
            tris[id].at = heap.emplace(1., id);
            scan(id);
        }
        for (int i = 0; i < max_vertices; ++i) {
            if (heap.begin()->first < max_error)
                break;
            ++iterations;
            Heap::iterator const first = top();
            tied_tops += heap.count(first->first) > 1 && first->first > 0;
            ScanTriangle const chosen = tris[first->second];
            sub.insert(chosen.candidate, first->second);
            std::vector<std::size_t> const changed(sub.changed.begin(), sub.changed.end());
            noop_insertions += changed.empty();
            for (std::size_t id : changed) {
                if (id > tris.size() - 1) {
                    tris.emplace_back();
                    tris[id].at = heap.emplace(DBL_MAX, id);
                }
                load(id);
                scan(id);
            }
        }
    }
};

// S11: TriangleMesh::delete_invalid_faces
void delete_invalid_faces(std::vector<uint32_t> &f)
{
    auto invalid = [&](std::size_t i) { return f[i] == f[i + 1] && f[i + 1] == f[i + 2]; };
    std::size_t vi = 0, ii = f.size();
    while (vi < ii) {
        while (vi < ii && !invalid(vi))
            vi += 3;
        ii -= 3;
        while (vi < ii && invalid(ii))
            ii -= 3;
        if (vi >= ii)
            break;
        for (int k = 0; k < 3; ++k)
            std::swap(f[vi + k], f[ii + k]);
    }
    f.resize(vi);
}

// What a view's run met (optional, += so that views add up): [0] faces S10's
// zero-depth clause removes, [1] faces its edge-ratio clause removes, [2] / [3]
// faces whose k-th triangle has exactly 4 / 5 zero depths, [4] faces whose
// k-th triangle is not their own, [5] faces with an edge ratio in [0.1, 0.2),
// [6] iterations that chose among equal keys, [7] scans with equal best
// distances, [8] no-op insertions, [9] the most rows of a scanned triangle
// (a maximum), [10] iterations, [11] maps with a valid depth
enum { SSTAT_ZERO = 0, SSTAT_RATIO = 1, SSTAT_FOUR = 2, SSTAT_FIVE = 3, SSTAT_OTHER = 4,
    SSTAT_NEAR = 5, SSTAT_TIED_TOPS = 6, SSTAT_TIED_SCANS = 7, SSTAT_NOOP = 8, SSTAT_ROWS = 9,
    SSTAT_ITERATIONS = 10, SSTAT_VALID = 11, SSTAT_COUNT = 12 };

void loop_stats(Greedy const &g, int64_t *stats)
{
    if (stats == nullptr)
        return;
    stats[SSTAT_TIED_TOPS] += g.tied_tops;
    stats[SSTAT_TIED_SCANS] += g.tied_scans;
    stats[SSTAT_NOOP] += g.noop_insertions;
    stats[SSTAT_ROWS] = std::max<int64_t>(stats[SSTAT_ROWS], g.max_rows);
    stats[SSTAT_ITERATIONS] += g.iterations;
    bool valid = false;
    for (std::size_t i = 0; i < (std::size_t)g.w * g.h; ++i)
        valid = valid || g.dm[i] > 0;
    stats[SSTAT_VALID] += valid;
}

// S9-S12 for one view -> world positions, colours (bytes), faces
void clean_up(Greedy const &g, Camera const &cam, const uint8_t *image, int channels,
    std::vector<Vec3> &pos, std::vector<uint8_t> &rgb, std::vector<uint32_t> &faces,
    int variant = V_PINNED, int64_t *stats = nullptr)
{
    Subdivision &sub = const_cast<Subdivision &>(g.sub);
    // S9: float vertices, corners deleted (faces that use one go, ids shift by 4)
    std::vector<Vec3> v;
    for (std::size_t i = 4; i < sub.verts.size(); ++i)
        v.push_back(Vec3{ { (float)sub.verts[i].x, (float)sub.verts[i].y, (float)sub.verts[i].z } });
    faces.clear();
    std::vector<std::size_t> own;   // the triangle a face came from
    for (std::size_t t = 0; t < sub.tri_start.size(); ++t) {
        uint32_t ids[3];
        sub.triangle(t, ids);
        if (ids[0] < 4 || ids[1] < 4 || ids[2] < 4)
            continue;
        for (int k = 0; k < 3; ++k)
            faces.push_back(ids[k] - 4);
        own.push_back(t);
    }
    rgb.assign(3 * v.size(), 0);
    for (std::size_t i = 0; i < v.size(); ++i) {
        const uint8_t *px = image + ((std::size_t)(int)v[i][1] * g.w + (int)v[i][0]) * channels;
        rgb[3 * i] = px[0];
        rgb[3 * i + 1] = channels >= 3 ? px[1] : px[0];
        rgb[3 * i + 2] = channels >= 3 ? px[2] : px[0];
    }
    pos.resize(v.size());
    for (std::size_t i = 0; i < v.size(); ++i) {
        Vec3 const ray = mult(cam.invproj, Vec3{ { v[i][0] + 0.5f, v[i][1] + 0.5f, 1.0f } });
        float const len = std::sqrt(square_norm(ray));
        Vec3 pc;
        for (int k = 0; k < 3; ++k)
            pc[k] = ray[k] / len * v[i][2];
        for (int r = 0; r < 3; ++r) {
            float s = 0.0f;
            for (int k = 0; k < 3; ++k)
                s += cam.ctw[4 * r + k] * pc[k];
            s += cam.ctw[4 * r + 3] * 1.0f;
            pos[i][r] = s;
        }
    }
    // S10: face k against the k-th triangle by id
    auto edge = [&](uint32_t a, uint32_t b) {
        Vec3 d;
        for (int k = 0; k < 3; ++k)
            d[k] = pos[a][k] - pos[b][k];
        return std::sqrt(square_norm(d));
    };
    for (std::size_t f = 0; f < faces.size(); f += 3) {
        float const e1 = edge(faces[f], faces[f + 1]), e2 = edge(faces[f], faces[f + 2]),
            e3 = edge(faces[f + 1], faces[f + 2]);
        float const lo = std::min(e1, std::min(e2, e3)), hi = std::max(e1, std::max(e2, e3));
        int const zeros = g.tris[variant == V_S10_OWN_TRIANGLE ? own[f / 3] : f / 3].num_zero;
        bool const holes = variant == V_S10_GE4 ? zeros >= 4 : zeros > 4;
        if (stats != nullptr) {
            stats[SSTAT_ZERO] += holes;
            stats[SSTAT_RATIO] += lo / hi < 0.1;
            stats[SSTAT_FOUR] += zeros == 4;
            stats[SSTAT_FIVE] += zeros == 5;
            stats[SSTAT_OTHER] += own[f / 3] != f / 3;
            stats[SSTAT_NEAR] += lo / hi >= 0.1 && lo / hi < 0.2;
        }
        if (holes || lo / hi < 0.1)
            faces[f] = faces[f + 1] = faces[f + 2] = 0;
    }
    delete_invalid_faces(faces);   // S11
    // S12
    std::vector<uint32_t> map(pos.size(), 0xffffffffu);
    std::vector<bool> used(pos.size(), false);
    for (uint32_t id : faces)
        used[id] = true;
    std::size_t n = 0;
    for (std::size_t i = 0; i < pos.size(); ++i) {
        if (!used[i])
            continue;
        map[i] = (uint32_t)n;
        pos[n] = pos[i];
        for (int k = 0; k < 3; ++k)
            rgb[3 * n + k] = rgb[3 * i + k];
        ++n;
    }
    pos.resize(n);
    rgb.resize(3 * n);
    for (uint32_t &id : faces)
        id = map[id];
}

} // namespace

// S1-S8 on one depth map.  verts: (budget + 4) * 3 doubles, tris: (2 budget + 2)
// * 3 ids, nzero: 2 budget + 2; variant: 0, or the one rule of `Variant` to
// get wrong; stats: optional, SSTAT_COUNT entries.  -> loop iterations run.
extern "C" int64_t
simplify_ref_triangulate(int w, int h, const float *dm, int max_vertices, double max_error,
    double *verts, int64_t *n_verts, uint32_t *tris, int32_t *nzero, int64_t *n_tris,
    int variant, int64_t *stats)
{
    Greedy g;
    g.w = w;
    g.h = h;
    g.dm = dm;
    g.variant = variant;
    g.run(max_vertices, max_error);
    loop_stats(g, stats);
    for (std::size_t i = 0; i < g.sub.verts.size(); ++i) {
        verts[3 * i] = g.sub.verts[i].x;
        verts[3 * i + 1] = g.sub.verts[i].y;
        verts[3 * i + 2] = g.sub.verts[i].z;
    }
    *n_verts = (int64_t)g.sub.verts.size();
    for (std::size_t t = 0; t < g.sub.tri_start.size(); ++t) {
        g.sub.triangle(t, tris + 3 * t);
        nzero[t] = g.tris[t].num_zero;
    }
    *n_tris = (int64_t)g.sub.tri_start.size();
    return g.iterations;
}

// One view of generate_mesh with Options::simplify (S1-S13 up to the merge).
// Outputs hold up to w * h / 40 + 4 (or max_vertices + 4) vertices and twice as
// many faces; variant and stats as simplify_ref_triangulate; vclass (optional)
// gets MeshInfo's class per vertex.  -> number of vertices.
extern "C" int64_t
simplify_ref_view(int w, int h, float flen, const float *rot, const float *trans,
    const float *dm, const float *wnormals, const uint8_t *image, int channels,
    int max_vertices, double max_error, float *xyz, float *nrm, uint8_t *rgb_out,
    float *conf, float *val, uint32_t *faces_out, int64_t *n_faces, int variant,
    int64_t *stats, int32_t *vclass)
{
    Camera const cam = make_camera(w, h, flen, rot, trans);
    Greedy g;
    g.w = w;
    g.h = h;
    g.dm = dm;
    g.variant = variant;
    g.run(max_vertices, max_error);
    loop_stats(g, stats);
    std::vector<Vec3> verts;
    std::vector<uint8_t> rgb;
    std::vector<uint32_t> faces;
    clean_up(g, cam, image, channels, verts, rgb, faces, variant, stats);
    std::size_t const nv = verts.size();
    std::vector<VertexInfo> const info = mesh_info(nv, faces, variant);
    std::vector<float> confs;
    mesh_confidences(info, 4, confs, variant);
    for (std::size_t j = 0; j < nv; ++j) {
        float s = 0.0f;
        for (uint32_t k : info[j].verts) {
            Vec3 d;
            for (int i = 0; i < 3; ++i)
                d[i] = verts[j][i] - verts[k][i];
            s += std::sqrt(square_norm(d));
        }
        s /= static_cast<float>(info[j].verts.size());
        s *= 2.0f;
        val[j] = s;
        conf[j] = confs[j];
        if (vclass != nullptr)
            vclass[j] = info[j].vclass;
        for (int i = 0; i < 3; ++i) {
            xyz[3 * j + i] = verts[j][i];
            rgb_out[3 * j + i] = rgb[3 * j + i];
        }
        float p[3];
        for (int r = 0; r < 3; ++r) {
            float d = 0.0f;
            for (int k = 0; k < 3; ++k)
                d += cam.KR[3 * r + k] * verts[j][k];
            p[r] = d - cam.t[r];
        }
        float const qx = p[0] / p[2], qy = p[1] / p[2];
        float n[3] = { 0.0f, 0.0f, 0.0f };
        if (qx > -1.0f && qx < (float)w && qy > -1.0f && qy < (float)h) {
            int const x = (int)qx, y = (int)qy;
            for (int r = 0; r < 3; ++r)
                n[r] = wnormals[3 * ((std::size_t)y * w + x) + r];
        }
        for (int r = 0; r < 3; ++r)
            nrm[3 * j + r] = n[r];
    }
    std::memcpy(faces_out, faces.data(), faces.size() * sizeof(uint32_t));
    *n_faces = (int64_t)(faces.size() / 3);
    return (int64_t)nv;
}

// S8 alone: the pixels of triangle (a, b, c) in emission order -> their number
// (at most cap are written as x, y pairs).
extern "C" int64_t
simplify_ref_pixels(const double *abc, int32_t *xy, int64_t cap)
{
    PixelList px;
    pixels_for_triangle(P2{ abc[0], abc[1] }, P2{ abc[2], abc[3] }, P2{ abc[4], abc[5] }, px);
    for (std::size_t i = 0; i < px.size() && (int64_t)i < cap; ++i) {
        xy[2 * i] = px[i].first;
        xy[2 * i + 1] = px[i].second;
    }
    return (int64_t)px.size();
}

// S4 / S5 alone: n points inserted into the quad (lo, lo)-(hi, hi), each
// located from triangle 0.  tris: room for 2 n + 2 triangles; changed_sizes[i]:
// the size of the changed set of insertion i.  -> triangles.
extern "C" int64_t
simplify_ref_delaunay(double lo, double hi, int64_t n, const double *pts, uint32_t *tris,
    int32_t *changed_sizes, int64_t *n_verts)
{
    Subdivision s;
    s.initialize(P3{ lo, lo, 0 }, P3{ hi, lo, 0 }, P3{ lo, hi, 0 }, P3{ hi, hi, 0 });
    for (int64_t i = 0; i < n; ++i) {
        s.insert(P3{ pts[2 * i], pts[2 * i + 1], 0.0 }, 0);
        changed_sizes[i] = (int32_t)s.changed.size();
    }
    for (std::size_t t = 0; t < s.tri_start.size(); ++t)
        s.triangle(t, tris + 3 * t);
    *n_verts = (int64_t)s.verts.size();
    return (int64_t)s.tri_start.size();
}

// S6 alone: keys emplaced in the given order, then popped from begin()
extern "C" void
simplify_ref_heap_order(int64_t n, const double *keys, int64_t *order)
{
    Heap heap;
    for (int64_t i = 0; i < n; ++i)
        heap.emplace(keys[i], (std::size_t)i);
    for (int64_t i = 0; i < n; ++i) {
        order[i] = (int64_t)heap.begin()->second;
        heap.erase(heap.begin());
    }
}

// S11 alone, in place -> faces left
extern "C" int64_t
simplify_ref_delete_invalid_faces(int64_t m, uint32_t *faces)
{
    std::vector<uint32_t> f(faces, faces + 3 * m);
    delete_invalid_faces(f);
    std::memcpy(faces, f.data(), f.size() * sizeof(uint32_t));
    return (int64_t)(f.size() / 3);
}
