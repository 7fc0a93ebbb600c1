#include "mesh_generator.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <stdexcept>

#include "../../../include/smvs_hip.h"

namespace smvs_amd {

namespace {

void check_status(int rc, char const* what)
{
    if (rc != SMVS_OK)
        throw std::runtime_error(std::string(what) + ": " + smvs_last_error());
}

// `mesh` sized for nv vertices and nf faces and filled from `handle`, which is
// released here
void download_mesh(smvs_points* handle, int64_t nv, int64_t nf, TriangleMesh& mesh)
{
    mesh.xyz.resize(3 * (std::size_t)nv);
    mesh.normals.resize(3 * (std::size_t)nv);
    mesh.colors.resize(3 * (std::size_t)nv);
    mesh.confidences.resize((std::size_t)nv);
    mesh.faces.resize(3 * (std::size_t)nf);
    int const rc = smvs_points_download(handle, mesh.xyz.data(), mesh.normals.data(),
        mesh.colors.data(), mesh.confidences.data(), nullptr, mesh.faces.data());
    smvs_points_release(handle);
    check_status(rc, "smvs_points_download");
}

} // namespace

MeshGenerator::MeshGenerator(Options const& o) : opts(o)
{
    if (opts.simplify)
        throw std::invalid_argument("MeshGenerator: the simplified "
            "triangulation (--simplify) is not supported");
}

struct MeshGenerator::Inputs
{
    std::vector<SceneView const*> views;
    std::vector<FloatImage::Ptr> depth, normals, cut;
    std::vector<ByteImage::Ptr> color;
    std::vector<smvs_point_view> pv;
};

void
MeshGenerator::load_views(std::vector<SceneView> const& inputviews,
    std::string const& image_name, std::string const& dm_name, Inputs& in) const
{
    std::string const nm_name = dm_name + "N";
    for (SceneView const& v : inputviews) {
        if (!v.present || !v.has_image(dm_name) || !v.has_image(nm_name)
            || !v.has_image(image_name))
            continue;
        in.views.push_back(&v);
    }
    std::size_t const n = in.views.size();
    in.depth.resize(n);
    in.normals.resize(n);
    in.color.resize(n);
    in.cut.resize(n);
    in.pv.resize(n);
    for (std::size_t i = 0; i < n; ++i) {
        SceneView const& v = *in.views[i];
        in.depth[i] = load_mvei_float(v.image_path(dm_name));
        in.normals[i] = load_mvei_float(v.image_path(nm_name));
        in.color[i] = v.load_byte_image(image_name);
        int const w = in.depth[i]->width(), h = in.depth[i]->height();
        if (in.depth[i]->channels() != 1 || in.normals[i]->width() != w
            || in.normals[i]->height() != h || in.normals[i]->channels() != 3)
            throw std::invalid_argument("view " + std::to_string(v.id)
                + ": depth / normal maps do not match");
        // (depthmap_triangulate: "Color image dimension mismatch")
        if (in.color[i]->width() != w || in.color[i]->height() != h)
            throw std::invalid_argument("view " + std::to_string(v.id)
                + ": colour image dimension mismatch");
        in.cut[i] = FloatImage::create(w, h, 1);
        smvs_point_view& p = in.pv[i];
        p.width = w;
        p.height = h;
        p.flen = v.camera.flen;
        std::copy(v.camera.rot, v.camera.rot + 9, p.rot);
        std::copy(v.camera.trans, v.camera.trans + 3, p.trans);
        p.depth = in.depth[i]->begin();
        p.normals = in.normals[i]->begin();
        p.image = in.color[i]->begin();
        p.channels = in.color[i]->channels();
        p.cut_depth = opts.cut_surfaces ? in.cut[i]->begin() : nullptr;
    }
}

void
MeshGenerator::save_cut_maps(Inputs const& in) const
{
    if (opts.cut_surfaces)
        for (std::size_t i = 0; i < in.views.size(); ++i)
            save_mvei(in.views[i]->image_path("smvs-cut"),
                FloatImage::ConstPtr(in.cut[i]));
}

PointCloud::Ptr
MeshGenerator::generate_mesh(std::vector<SceneView> const& inputviews,
    std::string const& image_name, std::string const& dm_name)
{
    if (opts.create_triangle_mesh)
        throw std::invalid_argument("MeshGenerator::generate_mesh: the triangle "
            "mesh (create_triangle_mesh, --mesh) comes from generate_triangle_mesh");
    Inputs in;
    load_views(inputviews, image_name, dm_name, in);
    PointCloud::Ptr pset(new PointCloud);
    if (in.views.empty())
        return pset;
    smvs_points_options po;
    po.cut_surfaces = opts.cut_surfaces ? 1 : 0;
    po.use_aabb = opts.use_aabb ? 1 : 0;
    std::copy(opts.aabb_min, opts.aabb_min + 3, po.aabb_min);
    std::copy(opts.aabb_max, opts.aabb_max + 3, po.aabb_max);
    po.dd_factor = opts.dd_factor;
    po.want_faces = 0;
    smvs_points* handle = nullptr;
    int64_t n = 0;
    check_status(smvs_points_generate(opts.device, in.pv.data(), (int)in.pv.size(), &po,
        &handle, &n), "smvs_points_generate");
    pset->xyz.resize(3 * (std::size_t)n);
    pset->normals.resize(3 * (std::size_t)n);
    pset->colors.resize(3 * (std::size_t)n);
    pset->confidences.resize((std::size_t)n);
    pset->values.resize((std::size_t)n);
    int const rc = smvs_points_download(handle, pset->xyz.data(), pset->normals.data(),
        pset->colors.data(), pset->confidences.data(), pset->values.data(), nullptr);
    smvs_points_release(handle);
    check_status(rc, "smvs_points_download");
    save_cut_maps(in);
    return pset;
}

TriangleMesh::Ptr
MeshGenerator::generate_triangle_mesh(std::vector<SceneView> const& inputviews,
    std::string const& image_name, std::string const& dm_name)
{
    Inputs in;
    load_views(inputviews, image_name, dm_name, in);
    TriangleMesh::Ptr mesh(new TriangleMesh);
    if (in.views.empty())
        return mesh;
    smvs_mesh_options mo;
    mo.cut_surfaces = opts.cut_surfaces ? 1 : 0;
    mo.use_aabb = opts.use_aabb ? 1 : 0;
    std::copy(opts.aabb_min, opts.aabb_min + 3, mo.aabb_min);
    std::copy(opts.aabb_max, opts.aabb_max + 3, mo.aabb_max);
    mo.dd_factor = opts.dd_factor;
    smvs_points* handle = nullptr;
    int64_t nv = 0, nf = 0;
    check_status(smvs_mesh_generate(opts.device, in.pv.data(), (int)in.pv.size(), &mo,
        &handle, &nv, &nf), "smvs_mesh_generate");
    download_mesh(handle, nv, nf, *mesh);
    save_cut_maps(in);
    return mesh;
}

void
MeshGenerator::generate_simplified(std::vector<SceneView> const& inputviews,
    std::string const& image_name, std::string const& dm_name, bool create_triangle_mesh,
    PointCloud* points, TriangleMesh* mesh, int max_vertices, double max_error)
{
    if ((create_triangle_mesh ? (void*)mesh : (void*)points) == nullptr)
        throw std::invalid_argument("MeshGenerator::generate_simplified: no output");
    Inputs in;
    load_views(inputviews, image_name, dm_name, in);
    if (in.views.empty())
        return;
    smvs_simplify_options so;
    so.cut_surfaces = opts.cut_surfaces ? 1 : 0;
    so.use_aabb = opts.use_aabb ? 1 : 0;
    std::copy(opts.aabb_min, opts.aabb_min + 3, so.aabb_min);
    std::copy(opts.aabb_max, opts.aabb_max + 3, so.aabb_max);
    so.create_triangle_mesh = create_triangle_mesh ? 1 : 0;
    so.max_vertices = max_vertices;
    so.max_error = max_error;
    smvs_points* handle = nullptr;
    int64_t nv = 0, nf = 0;
    check_status(smvs_simplified_generate(opts.device, in.pv.data(), (int)in.pv.size(), &so,
        &handle, &nv, &nf), "smvs_simplified_generate");
    if (create_triangle_mesh) {
        download_mesh(handle, nv, nf, *mesh);
    } else {
        std::size_t const n = (std::size_t)nv;
        points->xyz.resize(3 * n);
        points->normals.resize(3 * n);
        points->colors.resize(3 * n);
        points->confidences.resize(n);
        points->values.resize(n);
        int const rc = smvs_points_download(handle, points->xyz.data(), points->normals.data(),
            points->colors.data(), points->confidences.data(), points->values.data(), nullptr);
        smvs_points_release(handle);
        check_status(rc, "smvs_points_download");
    }
    save_cut_maps(in);
}

namespace {

// the grid of generate_fused from its box: [lo, hi] is the settings' AABB, or
// the bounds of the depth maps' points, which are padded here
smvs_tsdf_options
fused_grid(MeshGenerator::Options const& opts, MeshGenerator::FusedOptions const& fused,
    float* lo, float* hi)
{
    for (int a = 0; a < 3; ++a)
        if (!(lo[a] <= hi[a]))
            throw std::invalid_argument(opts.use_aabb
                ? "generate_fused: the box is empty"
                : "generate_fused: the depth maps hold no valid pixel");
    auto longest = [&]() {
        return std::max(hi[0] - lo[0], std::max(hi[1] - lo[1], hi[2] - lo[2]));
    };
    float voxel = fused.voxel_size;
    if (!opts.use_aabb) {
        // the bounds are padded by the truncation distance; where that is 3
        // voxels of a voxel size that follows from the padded box:
        // voxel = (side + 6 voxel) / resolution
        float pad = fused.trunc;
        if (pad <= 0.0f) {
            if (voxel <= 0.0f)
                voxel = longest() / (float)(fused.resolution - 6);
            pad = 3.0f * voxel;
        }
        for (int a = 0; a < 3; ++a) {
            lo[a] -= pad;
            hi[a] += pad;
        }
    }
    if (voxel <= 0.0f)
        voxel = longest() / (float)fused.resolution;
    smvs_tsdf_options to;
    to.cut_surfaces = opts.cut_surfaces ? 1 : 0;
    to.voxel_size = voxel;
    to.trunc = fused.trunc;
    to.min_weight = fused.min_weight;
    for (int a = 0; a < 3; ++a) {
        to.origin[a] = lo[a];
        to.dims[a] = std::max(2, (int)std::ceil((hi[a] - lo[a]) / voxel));
    }
    return to;
}

// the fused mesh behind `handle` (released here), cleaned when asked for
TriangleMesh::Ptr
fused_result(MeshGenerator::Options const& opts, MeshGenerator::FusedOptions const& fused,
    smvs_points* handle, int64_t nv, int64_t nf, smvs_mesh_clean_stats* clean_stats)
{
    if (fused.clean) {
        smvs_mesh_clean_options co;
        co.threshold = fused.clean_threshold;
        co.percentile = fused.clean_percentile;
        co.component_size = fused.clean_component_size;
        co.keep_unreferenced = fused.clean_keep_unreferenced ? 1 : 0;
        smvs_mesh_clean_stats st = {};
        smvs_points* cleaned = nullptr;
        int const rc = smvs_mesh_clean_handle(opts.device, handle, &co, nullptr, nullptr,
            nullptr, &st, &cleaned, &nv, &nf);
        smvs_points_release(handle);
        check_status(rc, "smvs_mesh_clean_handle");
        handle = cleaned;
        if (clean_stats != nullptr)
            *clean_stats = st;
    }
    TriangleMesh::Ptr mesh(new TriangleMesh);
    download_mesh(handle, nv, nf, *mesh);
    return mesh;
}

// What generate_fused refuses in its options, stated once.  Each path asks at
// the point where it has always asked: the unbatched
// one after it has found a usable view, the batched ones before they load any.
void
check_fused_options(MeshGenerator::FusedOptions const& fused)
{
    if (fused.voxel_size <= 0.0f && fused.resolution < 8)
        throw std::invalid_argument("generate_fused: resolution must be at least 8");
    if (fused.sparse && fused.voxel_size <= 0.0f && fused.resolution > 4096)
        throw std::invalid_argument("generate_fused: resolution must be at most 4096");
    if (!fused.sparse && fused.max_bricks > 0)
        throw std::invalid_argument("generate_fused: max_bricks belongs to sparse");
    if (!fused.sparse && fused.cull)
        throw std::invalid_argument("generate_fused: cull belongs to sparse");
}

} // namespace

// The persistent volume behind a batched generate_fused, released on scope
// exit.  With marks_first every batch is marked before the first is integrated.
struct FusedBatchVolume
{
    bool marks_first = false;
    virtual ~FusedBatchVolume() {}
    virtual void create(int device, smvs_tsdf_options const& to) = 0;
    virtual void mark(std::vector<smvs_point_view> const&, int /*cut*/) {}
    virtual void integrate(std::vector<smvs_point_view> const& pv, int cut) = 0;
    virtual void extract(int min_weight, smvs_points** handle, int64_t* nv, int64_t* nf) = 0;
};

namespace {

// smvs_tsdf_volume
struct DenseBatchVolume : FusedBatchVolume
{
    smvs_tsdf_volume* v = nullptr;
    ~DenseBatchVolume() { smvs_tsdf_volume_release(v); }
    void create(int device, smvs_tsdf_options const& to) override
    {
        smvs_tsdf_volume_options vo;
        std::copy(to.origin, to.origin + 3, vo.origin);
        std::copy(to.dims, to.dims + 3, vo.dims);
        vo.voxel_size = to.voxel_size;
        vo.trunc = to.trunc;
        check_status(smvs_tsdf_volume_create(device, &vo, &v), "smvs_tsdf_volume_create");
    }
    void integrate(std::vector<smvs_point_view> const& pv, int cut) override
    {
        check_status(smvs_tsdf_volume_integrate(v, pv.data(), (int)pv.size(), cut),
            "smvs_tsdf_volume_integrate");
    }
    void extract(int min_weight, smvs_points** handle, int64_t* nv, int64_t* nf) override
    {
        check_status(smvs_tsdf_volume_extract(v, min_weight, nullptr, nullptr, handle, nv, nf),
            "smvs_tsdf_volume_extract");
    }
};

// smvs_tsdf_sparse_volume: every mark precedes the
// first integrate and nothing grows, so no brick is late
struct SparseBatchVolume : FusedBatchVolume
{
    smvs_tsdf_sparse_volume* v = nullptr;
    int64_t max_bricks;
    int cull;
    explicit SparseBatchVolume(MeshGenerator::FusedOptions const& fused)
        : max_bricks(fused.max_bricks), cull(fused.cull ? 1 : 0) { marks_first = true; }
    ~SparseBatchVolume() { smvs_tsdf_sparse_volume_release(v); }
    void create(int device, smvs_tsdf_options const& to) override
    {
        smvs_tsdf_sparse_volume_options vo;
        std::copy(to.origin, to.origin + 3, vo.origin);
        std::copy(to.dims, to.dims + 3, vo.dims);
        vo.voxel_size = to.voxel_size;
        vo.trunc = to.trunc;
        vo.max_bricks = max_bricks;
        check_status(smvs_tsdf_sparse_volume_create(device, &vo, &v),
            "smvs_tsdf_sparse_volume_create");
    }
    void mark(std::vector<smvs_point_view> const& pv, int cut) override
    {
        check_status(smvs_tsdf_sparse_volume_mark(v, pv.data(), (int)pv.size(), cut, cull),
            "smvs_tsdf_sparse_volume_mark");
    }
    void integrate(std::vector<smvs_point_view> const& pv, int cut) override
    {
        check_status(smvs_tsdf_sparse_volume_integrate(v, pv.data(), (int)pv.size(), cut, 0, 0),
            "smvs_tsdf_sparse_volume_integrate");
    }
    void extract(int min_weight, smvs_points** handle, int64_t* nv, int64_t* nf) override
    {
        check_status(smvs_tsdf_sparse_volume_extract(v, min_weight, nullptr, nullptr, nullptr,
            handle, nv, nf), "smvs_tsdf_sparse_volume_extract");
    }
};

} // namespace

TriangleMesh::Ptr
MeshGenerator::generate_fused(std::vector<SceneView> const& inputviews,
    std::string const& image_name, std::string const& dm_name, FusedOptions const& fused,
    smvs_mesh_clean_stats* clean_stats)
{
    if (fused.batch_views < 0)
        throw std::invalid_argument("generate_fused: batch_views must not be negative");
    if (fused.batch_views > 0) {
        if (fused.sparse)
            throw std::invalid_argument("generate_fused: batch_views belongs to the dense volume");
        DenseBatchVolume volume;
        return generate_fused_batched(inputviews, image_name, dm_name, fused,
            (std::size_t)fused.batch_views, volume, clean_stats);
    }
    if (fused.sparse_batch_views < 0)
        throw std::invalid_argument("generate_fused: sparse_batch_views must not be negative");
    if (fused.sparse_batch_views > 0) {
        if (!fused.sparse)
            throw std::invalid_argument("generate_fused: sparse_batch_views belongs to sparse");
        SparseBatchVolume volume(fused);
        return generate_fused_batched(inputviews, image_name, dm_name, fused,
            (std::size_t)fused.sparse_batch_views, volume, clean_stats);
    }
    Inputs in;
    load_views(inputviews, image_name, dm_name, in);
    if (in.views.empty())
        return TriangleMesh::Ptr(new TriangleMesh);
    check_fused_options(fused);
    int const n = (int)in.pv.size();
    float lo[3], hi[3];
    if (opts.use_aabb) {
        std::copy(opts.aabb_min, opts.aabb_min + 3, lo);
        std::copy(opts.aabb_max, opts.aabb_max + 3, hi);
    } else {
        check_status(smvs_tsdf_bounds(opts.device, in.pv.data(), n,
            opts.cut_surfaces ? 1 : 0, lo, hi), "smvs_tsdf_bounds");
    }
    smvs_tsdf_options const to = fused_grid(opts, fused, lo, hi);
    smvs_points* handle = nullptr;
    int64_t nv = 0, nf = 0;
    if (fused.sparse && fused.cull) {
        smvs_tsdf_sparse_opts so;
        so.max_bricks = fused.max_bricks;
        so.cull = 1;
        check_status(smvs_tsdf_fuse_sparse_opts(opts.device, in.pv.data(), n, &to, &so, nullptr,
            nullptr, nullptr, nullptr, nullptr, &handle, &nv, &nf),
            "smvs_tsdf_fuse_sparse_opts");
    } else if (fused.sparse) {
        smvs_tsdf_sparse_options so;
        so.max_bricks = fused.max_bricks;
        check_status(smvs_tsdf_fuse_sparse(opts.device, in.pv.data(), n, &to, &so, nullptr,
            nullptr, nullptr, nullptr, &handle, &nv, &nf), "smvs_tsdf_fuse_sparse");
    } else
        check_status(smvs_tsdf_fuse(opts.device, in.pv.data(), n, &to, nullptr, nullptr,
            &handle, &nv, &nf), "smvs_tsdf_fuse");
    return fused_result(opts, fused, handle, nv, nf, clean_stats);
}

// generate_fused with FusedOptions::batch_views or ::sparse_batch_views: `step`
// consecutive scene views are loaded at a time, once per pass -- for the bounds
// (skipped with use_aabb), for the marks where the volume has them, and for the
// integration into the persistent volume.  The usable views of the batches, one
// after the other, are the list generate_fused loads at once; the cut, when on,
// acts within a batch.
TriangleMesh::Ptr
MeshGenerator::generate_fused_batched(std::vector<SceneView> const& inputviews,
    std::string const& image_name, std::string const& dm_name, FusedOptions const& fused,
    std::size_t step, FusedBatchVolume& volume, smvs_mesh_clean_stats* clean_stats)
{
    check_fused_options(fused);
    int const cut = opts.cut_surfaces ? 1 : 0;
    // calls `use` with the view records of every batch that has a usable view
    auto for_batches = [&](auto use) {
        for (std::size_t at = 0; at < inputviews.size(); at += step) {
            std::vector<SceneView> const batch(inputviews.begin() + at,
                inputviews.begin() + std::min(inputviews.size(), at + step));
            Inputs in;
            load_views(batch, image_name, dm_name, in);
            if (!in.views.empty())
                use(in.pv);
        }
    };
    float lo[3], hi[3];
    std::size_t usable = 0;
    if (opts.use_aabb) {
        std::copy(opts.aabb_min, opts.aabb_min + 3, lo);
        std::copy(opts.aabb_max, opts.aabb_max + 3, hi);
    } else {
        // the union's box: min and max are exact, so the order does not matter
        for (int a = 0; a < 3; ++a) {
            lo[a] = INFINITY;
            hi[a] = -INFINITY;
        }
        for_batches([&](std::vector<smvs_point_view> const& pv) {
            float blo[3], bhi[3];
            check_status(smvs_tsdf_bounds(opts.device, pv.data(), (int)pv.size(), cut, blo, bhi),
                "smvs_tsdf_bounds");
            usable += pv.size();
            for (int a = 0; a < 3; ++a) {
                lo[a] = std::fmin(lo[a], blo[a]);
                hi[a] = std::fmax(hi[a], bhi[a]);
            }
        });
        if (usable == 0)
            return TriangleMesh::Ptr(new TriangleMesh);
    }
    smvs_tsdf_options const to = fused_grid(opts, fused, lo, hi);
    volume.create(opts.device, to);
    // (with use_aabb this pass is the first to learn whether a view is usable)
    usable = 0;
    for_batches([&](std::vector<smvs_point_view> const& pv) {
        if (volume.marks_first)
            volume.mark(pv, cut);
        else
            volume.integrate(pv, cut);
        usable += pv.size();
    });
    if (usable == 0)
        return TriangleMesh::Ptr(new TriangleMesh);
    if (volume.marks_first)
        for_batches([&](std::vector<smvs_point_view> const& pv) { volume.integrate(pv, cut); });
    smvs_points* handle = nullptr;
    int64_t nv = 0, nf = 0;
    volume.extract(to.min_weight, &handle, &nv, &nf);
    return fused_result(opts, fused, handle, nv, nf, clean_stats);
}

void
save_ply_points(std::string const& path, PointCloud const& points)
{
    std::size_t const n = points.size();
    if (points.xyz.size() != 3 * n || points.normals.size() != 3 * n
        || points.colors.size() != 3 * n || points.values.size() != n)
        throw std::invalid_argument("save_ply_points: attribute sizes differ");
    std::ofstream out(path.c_str(), std::ios::binary);
    if (!out)
        throw std::runtime_error("save_ply_points: cannot open " + path);
    out << "ply\n"
        << "format binary_little_endian 1.0\n"
        << "comment Export generated by smvs_amd\n"
        << "element vertex " << n << "\n"
        << "property float x\nproperty float y\nproperty float z\n"
        << "property float nx\nproperty float ny\nproperty float nz\n"
        << "property uchar red\nproperty uchar green\nproperty uchar blue\n"
        << "property float confidence\n"
        << "property float value\n"
        << "element face 0\n"
        << "property list uchar int vertex_indices\n"
        << "end_header\n";
    // 35 bytes per vertex, interleaved in chunks (the hosts are little endian)
    std::size_t const chunk = 1 << 16;
    std::vector<char> buf(chunk * 35);
    for (std::size_t at = 0; at < n; at += chunk) {
        std::size_t const m = std::min(chunk, n - at);
        char* p = buf.data();
        for (std::size_t i = at; i < at + m; ++i) {
            std::memcpy(p, &points.xyz[3 * i], 12);
            std::memcpy(p + 12, &points.normals[3 * i], 12);
            std::memcpy(p + 24, &points.colors[3 * i], 3);
            std::memcpy(p + 27, &points.confidences[i], 4);
            std::memcpy(p + 31, &points.values[i], 4);
            p += 35;
        }
        out.write(buf.data(), (std::streamsize)(m * 35));
    }
    if (!out)
        throw std::runtime_error("save_ply_points: write failed: " + path);
}

void
save_ply_mesh(std::string const& path, TriangleMesh const& mesh)
{
    std::size_t const n = mesh.size(), m = mesh.num_faces();
    if (mesh.xyz.size() != 3 * n || mesh.normals.size() != 3 * n
        || mesh.colors.size() != 3 * n || mesh.faces.size() != 3 * m)
        throw std::invalid_argument("save_ply_mesh: attribute sizes differ");
    if (n > (std::size_t)INT32_MAX)
        throw std::invalid_argument("save_ply_mesh: vertex ids exceed int32");
    for (uint32_t id : mesh.faces)
        if (id >= n)
            throw std::invalid_argument("save_ply_mesh: face references no vertex");
    std::ofstream out(path.c_str(), std::ios::binary);
    if (!out)
        throw std::runtime_error("save_ply_mesh: cannot open " + path);
    out << "ply\n"
        << "format binary_little_endian 1.0\n"
        << "comment Export generated by smvs_amd\n"
        << "element vertex " << n << "\n"
        << "property float x\nproperty float y\nproperty float z\n"
        << "property float nx\nproperty float ny\nproperty float nz\n"
        << "property uchar red\nproperty uchar green\nproperty uchar blue\n"
        << "property float confidence\n"
        << "element face " << m << "\n"
        << "property list uchar int vertex_indices\n"
        << "end_header\n";
    // 31 bytes per vertex, 13 per face, in chunks (the hosts are little endian)
    std::size_t const chunk = 1 << 16;
    std::vector<char> buf(chunk * 31);
    for (std::size_t at = 0; at < n; at += chunk) {
        std::size_t const k = std::min(chunk, n - at);
        char* p = buf.data();
        for (std::size_t i = at; i < at + k; ++i) {
            std::memcpy(p, &mesh.xyz[3 * i], 12);
            std::memcpy(p + 12, &mesh.normals[3 * i], 12);
            std::memcpy(p + 24, &mesh.colors[3 * i], 3);
            std::memcpy(p + 27, &mesh.confidences[i], 4);
            p += 31;
        }
        out.write(buf.data(), (std::streamsize)(k * 31));
    }
    for (std::size_t at = 0; at < m; at += chunk) {
        std::size_t const k = std::min(chunk, m - at);
        char* p = buf.data();
        for (std::size_t i = at; i < at + k; ++i) {
            *p = 3;
            std::memcpy(p + 1, &mesh.faces[3 * i], 12);
            p += 13;
        }
        out.write(buf.data(), (std::streamsize)(k * 13));
    }
    if (!out)
        throw std::runtime_error("save_ply_mesh: write failed: " + path);
}

namespace {

// the scene's views of the settings and the embedding names smvsrecon's main
// hands over (:502-515)
struct SceneInputs
{
    Scene::Ptr scene;
    std::vector<SceneView> views;
    std::string input_name, dm_name;
};

SceneInputs
scene_inputs(std::string const& scene_path, PointCloudSettings const& conf)
{
    SceneInputs s;
    s.scene = Scene::create(scene_path);
    std::vector<SceneView>& all = s.scene->get_views();
    if (conf.view_ids.empty())
        s.views = all;
    else
        for (int id : conf.view_ids) {
            if (id < 0 || id >= (int)all.size())
                throw std::invalid_argument("no view " + std::to_string(id));
            s.views.push_back(all[(std::size_t)id]);
        }
    s.input_name = conf.input_scale > 0
        ? "undist-L" + std::to_string(conf.input_scale) : conf.image_embedding;
    s.dm_name = std::string(conf.use_shading ? "smvs-S" : "smvs-B")
        + std::to_string(conf.input_scale);
    return s;
}

MeshGenerator::Options
generator_options(PointCloudSettings const& conf)
{
    MeshGenerator::Options mo;
    mo.cut_surfaces = conf.cut_surface;
    mo.device = conf.device;
    mo.use_aabb = conf.use_aabb;
    std::copy(conf.aabb_min, conf.aabb_min + 3, mo.aabb_min);
    std::copy(conf.aabb_max, conf.aabb_max + 3, mo.aabb_max);
    return mo;
}

// :326-335
std::string
output_name(Scene const& scene, PointCloudSettings const& conf, bool mesh)
{
    std::string meshname = "smvs-";
    if (mesh)
        meshname += "m-";
    meshname += conf.use_shading ? "S" : "B";
    meshname += std::to_string(conf.input_scale) + ".ply";
    return scene.get_path() + "/" + meshname;
}

} // namespace

std::string
generate_scene_point_cloud(std::string const& scene_path,
    PointCloudSettings const& conf, std::size_t* n_points)
{
    if (conf.create_triangle_mesh)
        throw std::invalid_argument("--mesh (create_triangle_mesh) is not supported");
    if (conf.simplify)
        throw std::invalid_argument("--simplify is not supported");
    SceneInputs const in = scene_inputs(scene_path, conf);
    MeshGenerator meshgen(generator_options(conf));
    PointCloud::Ptr points = meshgen.generate_mesh(in.views, in.input_name, in.dm_name);
    std::string const meshname = output_name(*in.scene, conf, false);
    save_ply_points(meshname, *points);
    if (n_points != nullptr)
        *n_points = points->size();
    return meshname;
}

std::string
generate_scene_mesh(std::string const& scene_path, PointCloudSettings const& conf,
    std::size_t* n_vertices, std::size_t* n_faces)
{
    if (conf.simplify)
        throw std::invalid_argument("--simplify is not supported");
    SceneInputs const in = scene_inputs(scene_path, conf);
    MeshGenerator::Options mo = generator_options(conf);
    mo.create_triangle_mesh = true;
    MeshGenerator meshgen(mo);
    TriangleMesh::Ptr mesh = meshgen.generate_triangle_mesh(in.views, in.input_name,
        in.dm_name);
    std::string const meshname = output_name(*in.scene, conf, true);
    save_ply_mesh(meshname, *mesh);
    if (n_vertices != nullptr)
        *n_vertices = mesh->size();
    if (n_faces != nullptr)
        *n_faces = mesh->num_faces();
    return meshname;
}

std::string
generate_scene_simplified(std::string const& scene_path, PointCloudSettings const& conf,
    std::size_t* n_vertices, std::size_t* n_faces)
{
    SceneInputs const in = scene_inputs(scene_path, conf);
    MeshGenerator meshgen(generator_options(conf));
    std::string const meshname = output_name(*in.scene, conf, conf.create_triangle_mesh);
    std::size_t nv = 0, nf = 0;
    if (conf.create_triangle_mesh) {
        TriangleMesh mesh;
        meshgen.generate_simplified(in.views, in.input_name, in.dm_name, true, nullptr, &mesh);
        save_ply_mesh(meshname, mesh);
        nv = mesh.size();
        nf = mesh.num_faces();
    } else {
        PointCloud points;
        meshgen.generate_simplified(in.views, in.input_name, in.dm_name, false, &points,
            nullptr);
        save_ply_points(meshname, points);
        nv = points.size();
    }
    if (n_vertices != nullptr)
        *n_vertices = nv;
    if (n_faces != nullptr)
        *n_faces = nf;
    return meshname;
}

std::string
generate_scene_fused(std::string const& scene_path, PointCloudSettings const& conf,
    MeshGenerator::FusedOptions const& fused, std::size_t* n_vertices, std::size_t* n_faces,
    smvs_mesh_clean_stats* clean_stats)
{
    SceneInputs const in = scene_inputs(scene_path, conf);
    MeshGenerator meshgen(generator_options(conf));
    TriangleMesh::Ptr mesh = meshgen.generate_fused(in.views, in.input_name, in.dm_name, fused,
        clean_stats);
    std::string const meshname = in.scene->get_path()
        + (fused.clean ? "/smvs-clean-" : "/smvs-fused-")
        + (conf.use_shading ? "S" : "B") + std::to_string(conf.input_scale) + ".ply";
    save_ply_mesh(meshname, *mesh);
    if (n_vertices != nullptr)
        *n_vertices = mesh->size();
    if (n_faces != nullptr)
        *n_faces = mesh->num_faces();
    return meshname;
}

} // namespace smvs_amd
