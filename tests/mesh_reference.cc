// Serial CPU restatement of smvsrecon --mesh after the merge (rows M1-M6 of
// DESIGN.md section 9.5): delete_vertices_fix_faces with the AABB clip list,
// recalc_normals' angle-weighted vertex normals and save_ply_mesh with
// smvsrecon's options.  Its input is the merged mesh of
// tests/points_reference.cc (positions, colours, confidences, faces), which
// already is mesh_merge's result (M1).  Test infrastructure only: compiled by
// tests/mesh_ref.py with g++ -O2 -ffp-contract=off and loaded through ctypes;
// it shares no source with the HIP kernels.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

namespace {

struct Vec3 {
    float v[3];
    float &operator[](int i) { return v[i]; }
    float operator[](int i) const { return v[i]; }
};

Vec3 operator-(Vec3 const &a, Vec3 const &b)
{
    return Vec3{ { a[0] - b[0], a[1] - b[1], a[2] - b[2] } };
}

Vec3 operator-(Vec3 const &a)
{
    return Vec3{ { -a[0], -a[1], -a[2] } };
}

// math::Vector::dot: 0 + x0 y0 + x1 y1 + x2 y2 (P4)
float dot(Vec3 const &a, Vec3 const &b)
{
    float s = 0.0f;
    for (int i = 0; i < 3; ++i)
        s += a[i] * b[i];
    return s;
}

float norm(Vec3 const &a)
{
    return std::sqrt(dot(a, a));
}

Vec3 cross(Vec3 const &a, Vec3 const &b)
{
    return Vec3{ { a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2],
        a[0] * b[1] - a[1] * b[0] } };
}

// M4's clamp before the arc cosine
float clamp_unit(float x)
{
    return x < -1.0f ? -1.0f : (x > 1.0f ? 1.0f : x);
}

// M2: TriangleMesh::delete_vertices_fix_faces(dlist)
void delete_vertices_fix_faces(std::vector<bool> const &dlist, std::vector<Vec3> &verts,
    std::vector<uint8_t> &colors, std::vector<float> &confs, std::vector<uint32_t> &faces)
{
    // (b) the new id of every vertex: its id minus the deleted ones before it
    std::vector<uint32_t> shift(verts.size());
    uint32_t deleted = 0;
    for (std::size_t i = 0; i < verts.size(); ++i) {
        shift[i] = deleted;
        if (dlist[i])
            ++deleted;
    }
    // (a) faces that reference a deleted vertex go, the rest keep their order
    std::vector<uint32_t> kept;
    kept.reserve(faces.size());
    for (std::size_t f = 0; f + 2 < faces.size(); f += 3) {
        if (dlist[faces[f]] || dlist[faces[f + 1]] || dlist[faces[f + 2]])
            continue;
        for (int k = 0; k < 3; ++k)
            kept.push_back(faces[f + k] - shift[faces[f + k]]);
    }
    faces.swap(kept);
    // (c) vertices and attributes compacted in order; (d) unreferenced ones stay
    std::size_t j = 0;
    for (std::size_t i = 0; i < verts.size(); ++i) {
        if (dlist[i])
            continue;
        verts[j] = verts[i];
        for (int k = 0; k < 3; ++k)
            colors[3 * j + k] = colors[3 * i + k];
        confs[j] = confs[i];
        ++j;
    }
    verts.resize(j);
    colors.resize(3 * j);
    confs.resize(j);
}

// M3 / M4 for face (a, b, c): the unit face normal and the angle weights of
// its corners; -> false when fnl == 0 (the face adds nothing)
bool face_terms(Vec3 const &a, Vec3 const &b, Vec3 const &c, Vec3 &fn, float *w)
{
    Vec3 const ab = b - a, bc = c - b, ca = a - c;
    fn = cross(ab, -ca);
    float const fnl = norm(fn);
    if (fnl == 0.0f)
        return false;
    for (int k = 0; k < 3; ++k)
        fn[k] = fn[k] / fnl;
    w[0] = std::acos(clamp_unit(dot(ab, -ca) / (norm(ab) * norm(ca))));
    w[1] = std::acos(clamp_unit(dot(-ab, bc) / (norm(ab) * norm(bc))));
    w[2] = std::acos(clamp_unit(dot(ca, -bc) / (norm(ca) * norm(bc))));
    return true;
}

// M3-M5: TriangleMesh::recalc_normals (vertex normals only)
std::vector<Vec3> recalc_normals(std::vector<Vec3> const &verts,
    std::vector<uint32_t> const &faces)
{
    std::vector<Vec3> vn(verts.size(), Vec3{ { 0.0f, 0.0f, 0.0f } });
    for (std::size_t f = 0; f + 2 < faces.size(); f += 3) {
        Vec3 fn;
        float w[3];
        if (!face_terms(verts[faces[f]], verts[faces[f + 1]], verts[faces[f + 2]], fn, w))
            continue;
        // vn[a] += fn * wa, vn[b] += fn * wb, vn[c] += fn * wc
        for (int j = 0; j < 3; ++j)
            for (int k = 0; k < 3; ++k)
                vn[faces[f + j]][k] += fn[k] * w[j];
    }
    for (Vec3 &n : vn) {
        float const l = norm(n);
        if (l > 0.0f)
            for (int k = 0; k < 3; ++k)
                n[k] = n[k] / l;
    }
    return vn;
}

} // namespace

// The merged mesh (n vertices, m faces) -> M2 with smvsrecon's AABB list
// (use_aabb: any coordinate < lo or > hi, smvsrecon.cc:310-315), then M3-M5.
// Outputs have room for n vertices and m faces; -> vertices kept, *m_out faces.
extern "C" int64_t
mesh_ref_run(int64_t n, const float *xyz, const uint8_t *rgb, const float *conf,
    int64_t m, const uint32_t *faces, int use_aabb, const float *lo, const float *hi,
    float *xyz_out, float *nrm_out, uint8_t *rgb_out, float *conf_out,
    uint32_t *faces_out, int64_t *m_out)
{
    std::vector<Vec3> verts((size_t)n);
    for (int64_t i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k)
            verts[i][k] = xyz[3 * i + k];
    std::vector<uint8_t> colors(rgb, rgb + 3 * n);
    std::vector<float> confs(conf, conf + n);
    std::vector<uint32_t> f(faces, faces + 3 * m);
    if (use_aabb) {
        std::vector<bool> dlist((size_t)n, false);
        for (int64_t v = 0; v < n; ++v)
            for (int k = 0; k < 3; ++k)
                if (verts[v][k] < lo[k] || verts[v][k] > hi[k])
                    dlist[v] = true;
        delete_vertices_fix_faces(dlist, verts, colors, confs, f);
    }
    std::vector<Vec3> const vn = recalc_normals(verts, f);
    for (size_t i = 0; i < verts.size(); ++i)
        for (int k = 0; k < 3; ++k) {
            xyz_out[3 * i + k] = verts[i][k];
            nrm_out[3 * i + k] = vn[i][k];
        }
    std::memcpy(rgb_out, colors.data(), colors.size());
    std::memcpy(conf_out, confs.data(), confs.size() * sizeof(float));
    std::memcpy(faces_out, f.data(), f.size() * sizeof(uint32_t));
    *m_out = (int64_t)(f.size() / 3);
    return (int64_t)verts.size();
}

// M3 / M4 per face of a mesh: fn (m x 3), the corner weights (m x 3) and
// whether the face counts (fnl != 0; else fn and weights are left 0)
extern "C" void
mesh_ref_face_terms(int64_t n, const float *xyz, int64_t m, const uint32_t *faces,
    float *fn_out, float *w_out, int32_t *valid_out)
{
    (void)n;
    auto vert = [&](uint32_t i) {
        return Vec3{ { xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2] } };
    };
    for (int64_t f = 0; f < m; ++f) {
        Vec3 fn;
        float w[3] = { 0.0f, 0.0f, 0.0f };
        bool const ok = face_terms(vert(faces[3 * f]), vert(faces[3 * f + 1]),
            vert(faces[3 * f + 2]), fn, w);
        valid_out[f] = ok ? 1 : 0;
        for (int k = 0; k < 3; ++k) {
            fn_out[3 * f + k] = ok ? fn[k] : 0.0f;
            w_out[3 * f + k] = w[k];
        }
    }
}

// M6: save_ply_mesh with smvsrecon's options on a mesh without values: the
// header of P13 without `value`, `element face m`, then n vertex records of 31
// bytes and m face records of `uchar 3` + three little-endian int32.
// -> 0, or -1 when the file cannot be written.
extern "C" int
mesh_ref_save_ply(const char *path, int64_t n, const float *xyz, const float *nrm,
    const uint8_t *rgb, const float *conf, int64_t m, const uint32_t *faces)
{
    FILE *f = std::fopen(path, "wb");
    if (f == nullptr)
        return -1;
    std::fprintf(f, "ply\nformat binary_little_endian 1.0\n"
        "comment Export generated by smvs_amd\n"
        "element vertex %lld\n"
        "property float x\nproperty float y\nproperty float z\n"
        "property float nx\nproperty float ny\nproperty float nz\n"
        "property uchar red\nproperty uchar green\nproperty uchar blue\n"
        "property float confidence\n"
        "element face %lld\n"
        "property list uchar int vertex_indices\n"
        "end_header\n", (long long)n, (long long)m);
    for (int64_t i = 0; i < n; ++i) {
        std::fwrite(xyz + 3 * i, 4, 3, f);
        std::fwrite(nrm + 3 * i, 4, 3, f);
        std::fwrite(rgb + 3 * i, 1, 3, f);
        std::fwrite(conf + i, 4, 1, f);
    }
    for (int64_t i = 0; i < m; ++i) {
        unsigned char const three = 3;
        std::fwrite(&three, 1, 1, f);
        for (int k = 0; k < 3; ++k) {
            int32_t const id = (int32_t)faces[3 * i + k];
            std::fwrite(&id, 4, 1, f);
        }
    }
    return std::fclose(f) == 0 ? 0 : -1;
}
