// Serial CPU restatement of the point export of MeshGenerator::generate_mesh
// (lib/mesh_generator.cc:217-297) for one view, literal to the MVE loops it
// calls as DESIGN.md section 9 pins them: depthmap_triangulate with a lazy
// vertex index map and an explicit face list, MeshInfo's chained one-rings,
// depthmap_mesh_confidences' ring growth, the scale value and the normal
// lookup.  Test infrastructure only: compiled by tests/test_points_cpu.py with
// g++ -O2 -ffp-contract=off and loaded through ctypes; it shares no source
// with the HIP kernels.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <list>
#include <vector>

namespace {

struct Vec3 {
    float v[3];
    float &operator[](int i) { return v[i]; }
    float operator[](int i) const { return v[i]; }
};

// math::Matrix3f * Vec3f: ret[i] = 0 + m[i][0] v[0] + m[i][1] v[1] + m[i][2] v[2]
Vec3 mult(const float *m, Vec3 const &a)
{
    Vec3 r;
    for (int i = 0; i < 3; ++i) {
        float s = 0.0f;
        for (int j = 0; j < 3; ++j)
            s += m[3 * i + j] * a[j];
        r[i] = s;
    }
    return r;
}

float square_norm(Vec3 const &a)
{
    float s = 0.0f;
    for (int i = 0; i < 3; ++i)
        s += a[i] * a[i];
    return s;
}

struct Camera {
    int w, h;
    float K[9], invproj[9], rot[9], KR[9], t[3], ctw[12];
};

Camera make_camera(int w, int h, float flen, const float *rot, const float *trans)
{
    Camera c;
    c.w = w;
    c.h = h;
    float const fw = (float)w, fh = (float)h;
    float const dim = std::max(fw, fh);
    float const ax = flen * dim, ay = flen * dim;
    float const K[9] = { ax, 0, fw * 0.5f, 0, ay, fh * 0.5f, 0, 0, 1 };
    float const Ki[9] = { 1.0f / ax, 0, -fw * 0.5f / ax, 0, 1.0f / ay,
        -fh * 0.5f / ay, 0, 0, 1 };
    std::memcpy(c.K, K, sizeof(K));
    std::memcpy(c.invproj, Ki, sizeof(Ki));
    std::memcpy(c.rot, rot, sizeof(c.rot));
    for (int r = 0; r < 3; ++r)
        for (int q = 0; q < 3; ++q) {
            float s = 0.0f;
            for (int k = 0; k < 3; ++k)
                s += K[3 * r + k] * rot[3 * k + q];
            c.KR[3 * r + q] = s;
        }
    float pos[3];
    for (int r = 0; r < 3; ++r) {
        float s = 0.0f;
        for (int k = 0; k < 3; ++k)
            s += -rot[3 * k + r] * trans[k];
        pos[r] = s;
    }
    for (int r = 0; r < 3; ++r) {
        float s = 0.0f;
        for (int k = 0; k < 3; ++k)
            s += c.KR[3 * r + k] * pos[k];
        c.t[r] = s;
    }
    // fill_cam_to_world: [R^T | -R^T t]
    for (int r = 0; r < 3; ++r) {
        for (int k = 0; k < 3; ++k)
            c.ctw[4 * r + k] = rot[3 * k + r];
        c.ctw[4 * r + 3] = pos[r];
    }
    return c;
}

// pixel_3dpos: (invproj * (x + .5, y + .5, 1)).normalized() * depth
Vec3 pixel_3dpos(int x, int y, float depth, const float *invproj)
{
    Vec3 ray = mult(invproj, Vec3{ { (float)x + 0.5f, (float)y + 0.5f, 1.0f } });
    float const len = std::sqrt(square_norm(ray));
    Vec3 r;
    for (int i = 0; i < 3; ++i)
        r[i] = ray[i] / len * depth;
    return r;
}

float pixel_footprint(int x, int y, float depth, const float *invproj)
{
    Vec3 v = mult(invproj, Vec3{ { (float)x + 0.5f, (float)y + 0.5f, 1.0f } });
    return invproj[0] * depth / std::sqrt(square_norm(v));
}

// The rules a subtly wrong kernel would get wrong, one per value (0 = the
// pinned behaviour); tests/test_export_cases_cpu.py counts what each changes.
enum Variant {
    V_PINNED = 0,
    V_P2_TIE_LE = 1,          // P2: `<=` for `<`
    V_P3_GE = 2,              // P3: `>=` for `>`
    V_P3_FOOTPRINT_MAX = 3,   // P3: the footprint of i_max
    V_P3_NO_SQRT2 = 4,        // P3: no MATH_SQRT2 on the diagonals
    V_P8_PREPEND_FIRST = 5,   // P8: prepend tested before append
    V_P9_UNSORTED = 6,        // P9: complex list in face order, not sorted
    V_P10_COMPLEX_SEEDS = 7,  // P10: complex vertices start the rings too
    V_S6_LATEST = 8,          // S6: the latest stamp among equal keys
    V_S7_GE = 9,              // S7: `>=` for `>`
    V_S8_MULTIPLY = 10,       // S8: x = xa + r * dx for the repeated addition
    V_S10_GE4 = 11,           // S10: `>= 4` for `> 4`
    V_S10_OWN_TRIANGLE = 12,  // S10: the face's own triangle, not the k-th
    V_S3_NO_FALLBACK = 13,    // S3: a zero corner depth stays zero
};

// What the triangulation met (optional, += so that views add up):
// [0..15] blocks per corner mask, [16] P2 ties, [17] P3 edges tested,
// [18] of them discontinuities, [19..21] axis edges whose larger depth is the
// last float below / the float exactly at / the first float above the
// threshold, [22..24] the same for diagonals, [25] edges of two equal depths
enum { STAT_MASK = 0, STAT_TIES = 16, STAT_EDGES = 17, STAT_DISC = 18, STAT_AXIS = 19,
    STAT_DIAG = 22, STAT_EQUAL = 25, STAT_COUNT = 26 };

bool dm_is_depthdisc(const float *widths, const float *depths, float dd_factor,
    int i1, int i2, int variant = V_PINNED, int64_t *stats = nullptr)
{
    int i_min = i1, i_max = i2;
    if (depths[i2] < depths[i1])
        std::swap(i_min, i_max);
    bool const diagonal = i1 + i2 == 3;
    if (diagonal && variant != V_P3_NO_SQRT2)
        dd_factor *= 1.41421356237309504880;   // MATH_SQRT2
    float const diff = depths[i_max] - depths[i_min];
    float const limit = widths[variant == V_P3_FOOTPRINT_MAX ? i_max : i_min] * dd_factor;
    bool const disc = variant == V_P3_GE ? diff >= limit : diff > limit;
    if (stats != nullptr) {
        stats[STAT_EDGES] += 1;
        stats[STAT_DISC] += disc;
        stats[STAT_EQUAL] += depths[i1] == depths[i2];
        int64_t *side = stats + (diagonal ? STAT_DIAG : STAT_AXIS);
        // one float step of the larger depth reaches or crosses the threshold
        float const up = std::nextafter(depths[i_max], INFINITY) - depths[i_min];
        float const down = std::nextafter(depths[i_max], 0.0f) - depths[i_min];
        side[0] += diff < limit && up >= limit;
        side[1] += diff == limit;
        side[2] += diff > limit && down <= limit;
    }
    return disc;
}

void dm_make_triangle(std::vector<Vec3> &verts, std::vector<uint32_t> &faces,
    std::vector<uint32_t> &vidx, const float *dm, const float *invproj,
    int width, int i, const int *tverts)
{
    for (int j = 0; j < 3; ++j) {
        int const iidx = i + (tverts[j] % 2) + width * (tverts[j] / 2);
        int const x = iidx % width, y = iidx / width;
        if (vidx[iidx] == 0xffffffffu) {
            vidx[iidx] = (uint32_t)verts.size();
            verts.push_back(pixel_3dpos(x, y, dm[iidx], invproj));
        }
        faces.push_back(vidx[iidx]);
    }
}

void depthmap_triangulate(const float *dm, int width, int height,
    const float *invproj, float dd_factor, std::vector<Vec3> &verts,
    std::vector<uint32_t> &faces, std::vector<uint32_t> &vidx, int variant = V_PINNED,
    int64_t *stats = nullptr)
{
    vidx.assign((size_t)width * height, 0xffffffffu);
    int i = 0;
    for (int y = 0; y < height - 1; ++y, ++i)
        for (int x = 0; x < width - 1; ++x, ++i) {
            float const depths[4] = { dm[i], dm[i + 1], dm[i + width],
                dm[i + width + 1] };
            int mask = 0, pixels = 0;
            for (int j = 0; j < 4; ++j)
                if (depths[j] > 0.0f) {
                    mask |= 1 << j;
                    pixels += 1;
                }
            if (stats != nullptr)
                stats[STAT_MASK + mask] += 1;
            if (pixels < 3)
                continue;
            int tris[4][3] = { { 0, 2, 1 }, { 0, 3, 1 }, { 0, 2, 3 }, { 1, 2, 3 } };
            int tri[2] = { 0, 0 };
            switch (mask) {
            case 7: tri[0] = 1; break;
            case 11: tri[0] = 2; break;
            case 13: tri[0] = 3; break;
            case 14: tri[0] = 4; break;
            case 15: {
                float const ddiff1 = std::abs(depths[0] - depths[3]);
                float const ddiff2 = std::abs(depths[1] - depths[2]);
                if (stats != nullptr)
                    stats[STAT_TIES] += ddiff1 == ddiff2;
                if (variant == V_P2_TIE_LE ? ddiff1 <= ddiff2 : ddiff1 < ddiff2) {
                    tri[0] = 2;
                    tri[1] = 3;
                } else {
                    tri[0] = 1;
                    tri[1] = 4;
                }
                break;
            }
            default: continue;
            }
            if (dd_factor > 0.0f) {
                float widths[4] = { 0, 0, 0, 0 };
                for (int j = 0; j < 4; ++j) {
                    if (depths[j] == 0.0f)
                        continue;
                    widths[j] = pixel_footprint(x + (j % 2), y + (j / 2), depths[j], invproj);
                }
                for (int j = 0; j < 2 && tri[j] != 0; ++j) {
                    int *tv = tris[tri[j] - 1];
                    if (dm_is_depthdisc(widths, depths, dd_factor, tv[0], tv[1], variant, stats))
                        tri[j] = 0;
                    if (dm_is_depthdisc(widths, depths, dd_factor, tv[1], tv[2], variant, stats))
                        tri[j] = 0;
                    if (dm_is_depthdisc(widths, depths, dd_factor, tv[2], tv[0], variant, stats))
                        tri[j] = 0;
                }
            }
            for (int j = 0; j < 2; ++j) {
                if (tri[j] == 0)
                    continue;
                dm_make_triangle(verts, faces, vidx, dm, invproj, width, i, tris[tri[j] - 1]);
            }
        }
}

enum VertexClass { UNREF = 0, SIMPLE = 1, BORDER = 2, COMPLEX = 3 };

struct VertexInfo {
    int vclass = UNREF;
    std::vector<uint32_t> verts, faces;
};

struct Edge {
    uint32_t v1, v2, f;
};

// mve::MeshInfo::initialize / update_vertex
std::vector<VertexInfo> mesh_info(size_t n_verts, std::vector<uint32_t> const &faces,
    int variant = V_PINNED)
{
    std::vector<VertexInfo> info(n_verts);
    for (size_t i = 0, i3 = 0; i < faces.size() / 3; ++i)
        for (int j = 0; j < 3; ++j, ++i3)
            info[faces[i3]].faces.push_back((uint32_t)i);
    for (size_t v = 0; v < n_verts; ++v) {
        VertexInfo &vi = info[v];
        std::list<Edge> adj_temp;
        for (uint32_t f : vi.faces)
            for (int j = 0; j < 3; ++j)
                if (faces[3 * f + j] == v) {
                    adj_temp.push_back(Edge{ faces[3 * f + (j + 1) % 3],
                        faces[3 * f + (j + 2) % 3], f });
                    break;
                }
        if (adj_temp.empty()) {
            vi.vclass = UNREF;
            vi.verts.clear();
            vi.faces.clear();
            continue;
        }
        std::list<Edge> adj_sorted;
        adj_sorted.push_back(adj_temp.front());
        adj_temp.pop_front();
        while (!adj_temp.empty()) {
            uint32_t const front_id = adj_sorted.front().v1;
            uint32_t const back_id = adj_sorted.back().v2;
            bool appended = false;
            for (auto it = adj_temp.begin(); it != adj_temp.end(); ++it) {
                if (variant == V_P8_PREPEND_FIRST && it->v2 == front_id) {
                    adj_sorted.push_front(*it);
                    adj_temp.erase(it);
                    appended = true;
                    break;
                }
                if (it->v1 == back_id) {
                    adj_sorted.push_back(*it);
                    adj_temp.erase(it);
                    appended = true;
                    break;
                }
                if (it->v2 == front_id) {
                    adj_sorted.push_front(*it);
                    adj_temp.erase(it);
                    appended = true;
                    break;
                }
            }
            if (!appended)
                break;
        }
        if (!adj_temp.empty()) {
            vi.vclass = COMPLEX;
            vi.verts.clear();
            for (uint32_t f : vi.faces)
                for (int j = 0; j < 3; ++j)
                    if (faces[3 * f + j] != v)
                        vi.verts.push_back(faces[3 * f + j]);
            if (variant == V_P9_UNSORTED) {
                // first occurrences in face order
                std::vector<uint32_t> seen;
                for (uint32_t a : vi.verts)
                    if (std::find(seen.begin(), seen.end(), a) == seen.end())
                        seen.push_back(a);
                vi.verts = seen;
                continue;
            }
            std::sort(vi.verts.begin(), vi.verts.end());
            vi.verts.erase(std::unique(vi.verts.begin(), vi.verts.end()), vi.verts.end());
            continue;
        }
        vi.vclass = adj_sorted.front().v1 == adj_sorted.back().v2 ? SIMPLE : BORDER;
        vi.faces.clear();
        vi.verts.clear();
        for (Edge const &e : adj_sorted) {
            vi.faces.push_back(e.f);
            vi.verts.push_back(e.v1);
        }
        if (vi.vclass == BORDER)
            vi.verts.push_back(adj_sorted.back().v2);
    }
    return info;
}

// mve::geom::depthmap_mesh_confidences
void mesh_confidences(std::vector<VertexInfo> const &info, int iterations,
    std::vector<float> &confs, int variant = V_PINNED)
{
    confs.assign(info.size(), 1.0f);
    std::vector<size_t> vidx;
    for (size_t i = 0; i < info.size(); ++i)
        if (info[i].vclass == BORDER
            || (variant == V_P10_COMPLEX_SEEDS && info[i].vclass == COMPLEX)) {
            vidx.push_back(i);
            confs[i] = 0.0f;
        }
    for (int current = 0; current < iterations; ++current) {
        size_t const num_vertices = vidx.size();
        for (size_t i = 0; i < num_vertices; ++i) {
            std::vector<uint32_t> const &adj = info[vidx[i]].verts;
            for (uint32_t a : adj)
                if (confs[a] == 1.0f) {
                    vidx.push_back(a);
                    confs[a] = static_cast<float>(current + 1) / static_cast<float>(iterations);
                }
        }
        vidx.erase(vidx.begin(), vidx.begin() + num_vertices);
    }
}

} // namespace

// One view: dm (ray-length depth to triangulate), wnormals (world space),
// image (channels bytes per pixel).  Outputs hold up to w*h vertices and
// 2*(w-1)*(h-1) faces; vclass (optional) gets MeshInfo's class per vertex,
// stats (optional, STAT_COUNT entries) what the triangulation met; variant:
// 0, or the one rule of `Variant` to get wrong.  -> number of vertices.
extern "C" int64_t
points_ref_view(int w, int h, float flen, const float *rot, const float *trans,
    const float *dm, const float *wnormals, const uint8_t *image, int channels,
    float dd_factor, float *xyz, float *nrm, uint8_t *rgb, float *conf,
    float *val, uint32_t *faces_out, int64_t *n_faces, int32_t *vclass, int variant,
    int64_t *stats)
{
    Camera const cam = make_camera(w, h, flen, rot, trans);
    std::vector<Vec3> verts;
    std::vector<uint32_t> faces, vidx;
    depthmap_triangulate(dm, w, h, cam.invproj, dd_factor, verts, faces, vidx, variant, stats);
    // mesh_transform with fill_cam_to_world: Matrix4f::mult(v, 1)
    for (Vec3 &v : verts) {
        Vec3 r;
        for (int i = 0; i < 3; ++i) {
            float s = 0.0f;
            for (int j = 0; j < 3; ++j)
                s += cam.ctw[4 * i + j] * v[j];
            s += cam.ctw[4 * i + 3] * 1.0f;
            r[i] = s;
        }
        v = r;
    }
    size_t const nv = verts.size();
    std::vector<VertexInfo> const info = mesh_info(nv, faces, variant);
    std::vector<float> confs;
    mesh_confidences(info, 4, confs, variant);
    for (size_t i = 0; i < (size_t)w * h; ++i) {
        if (vidx[i] == 0xffffffffu)
            continue;
        const uint8_t *px = image + i * channels;
        uint8_t *c = rgb + 3 * (size_t)vidx[i];
        c[0] = px[0];
        c[1] = channels >= 3 ? px[1] : px[0];
        c[2] = channels >= 3 ? px[2] : px[0];
    }
    for (size_t j = 0; j < nv; ++j) {
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
        for (int i = 0; i < 3; ++i)
            xyz[3 * j + i] = verts[j][i];
        if (vclass != nullptr)
            vclass[j] = info[j].vclass;
        // ViewProjection::get_proj, (int) truncation, 0 outside the map
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
                n[r] = wnormals[3 * ((size_t)y * w + x) + r];
        }
        for (int r = 0; r < 3; ++r)
            nrm[3 * j + r] = n[r];
    }
    if (faces_out != nullptr)
        std::memcpy(faces_out, faces.data(), faces.size() * sizeof(uint32_t));
    if (n_faces != nullptr)
        *n_faces = (int64_t)(faces.size() / 3);
    return (int64_t)nv;
}

// P4 alone: the footprint of pixel (x, y) at depth d in a w x h view
extern "C" float
points_ref_footprint(int w, int h, float flen, int x, int y, float d)
{
    float const rot[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 }, trans[3] = { 0, 0, 0 };
    Camera const cam = make_camera(w, h, flen, rot, trans);
    return pixel_footprint(x, y, d, cam.invproj);
}
