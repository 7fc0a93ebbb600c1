// smvs::MeshGenerator's point-cloud and triangle-mesh paths (reference:
// lib/mesh_generator.h, lib/mesh_generator.cc:160-299) and smvsrecon's
// generate_mesh (app/smvsrecon.cc:278-343) on top of smvs_points_generate and
// smvs_mesh_generate, and the simplified triangulation (--simplify) on top of
// smvs_simplified_generate.  The cut, the triangulation and every per-vertex value
// run on the device; the host loads the embeddings, writes smvs-cut per view
// and streams the PLY file.
#pragma once

#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "../../../include/smvs_hip.h"   // smvs_mesh_clean_stats
#include "scene_io.h"

namespace smvs_amd {

// mve::TriangleMesh reduced to what the point export fills (SoA as the C ABI
// hands it back); colours as the bytes save_ply_mesh writes
struct PointCloud
{
    typedef std::shared_ptr<PointCloud> Ptr;
    std::vector<float> xyz, normals, confidences, values;
    std::vector<uint8_t> colors;
    std::size_t size(void) const { return confidences.size(); }
};

// mve::TriangleMesh as smvsrecon --mesh saves it:
// the point cloud's SoA without values, plus the face list (3 vertex ids per
// face); normals are recalc_normals' vertex normals
struct TriangleMesh
{
    typedef std::shared_ptr<TriangleMesh> Ptr;
    std::vector<float> xyz, normals, confidences;
    std::vector<uint8_t> colors;
    std::vector<uint32_t> faces;
    std::size_t size(void) const { return confidences.size(); }
    std::size_t num_faces(void) const { return faces.size() / 3; }
};

// the persistent volume behind a batched generate_fused (mesh_generator.cc)
struct FusedBatchVolume;

class MeshGenerator
{
public:
    struct Options
    {
        std::size_t num_threads = 0;        // (the device does the work)
        bool cut_surfaces = true;
        bool simplify = false;              // refused here: generate_simplified is the entry
        bool create_triangle_mesh = false;  // generate_mesh refuses it: use
                                            // generate_triangle_mesh
        int device = 0;
        float dd_factor = 5.0f;
        bool use_aabb = false;              // smvsrecon --aabb (:306-319)
        float aabb_min[3] = { 0, 0, 0 }, aabb_max[3] = { 0, 0, 0 };
    };

    explicit MeshGenerator(Options const& opts);
    // views lacking depth (dm_name), normals (dm_name + "N") or the image are
    // skipped (:165-180); writes smvs-cut.mvei per view when cutting (:222-226)
    PointCloud::Ptr generate_mesh(std::vector<SceneView> const& views,
        std::string const& image_name, std::string const& dm_name);
    // the create_triangle_mesh path (:279-282) with smvsrecon's AABB clip and
    // recalc_normals (app/smvsrecon.cc:306-324), on smvs_mesh_generate; views
    // and smvs-cut as generate_mesh
    TriangleMesh::Ptr generate_triangle_mesh(std::vector<SceneView> const& views,
        std::string const& image_name, std::string const& dm_name);

    // Options::simplify (approximate_triangulation per view, DESIGN.md section
    // 9.7) on smvs_simplified_generate: the point cloud (points != nullptr) or,
    // with create_triangle_mesh, the mesh of --mesh --simplify (mesh !=
    // nullptr); views and smvs-cut as generate_mesh.  max_vertices / max_error:
    // -1 = approximate_triangulation's defaults
    void generate_simplified(std::vector<SceneView> const& views,
        std::string const& image_name, std::string const& dm_name,
        bool create_triangle_mesh, PointCloud* points, TriangleMesh* mesh,
        int max_vertices = -1, double max_error = -1.0);

    // Not in the reference: the views' depth maps fused into ONE surface mesh
    // on smvs_tsdf_fuse.  The box is [aabb_min,
    // aabb_max] with use_aabb, else smvs_tsdf_bounds padded by the truncation
    // distance; dims[a] = max(2, (int)ceilf((hi[a] - lo[a]) / voxel_size)).
    // No smvs-cut is written.  With sparse the volume is smvs_tsdf_fuse_sparse's
    // (section 9.9): the same mesh in the brick order, and resolution (and
    // every dim) may go up to 4096.
    struct FusedOptions
    {
        float voxel_size = 0.0f;    // <= 0: the box's longest side / resolution
        int resolution = 256;
        float trunc = 0.0f;         // <= 0: 3 voxels
        int min_weight = 0;         // <= 0: 1
        bool sparse = false;
        int64_t max_bricks = 0;     // sparse only; <= 0: 1 << 20
        bool cull = false;          // sparse only: the brick cull in front of the
                                    // seed pass (section 9.10), the same mesh
        // the fused mesh (dense, sparse or sparse + cull) goes through
        // smvs_mesh_clean_handle (section 9.12) before it comes back; off:
        // the calls made are the ones above
        bool clean = false;
        float clean_threshold = 0.0f;       // meshclean -t; 0: off
        float clean_percentile = 0.0f;      // meshclean -p; 0: off
        int clean_component_size = 1000;    // meshclean -c
        bool clean_keep_unreferenced = false;
        // > 0 (dense only): only batch_views consecutive scene views are
        // loaded at a time, for the bounds and for the integration into a
        // persistent volume (smvs_tsdf_volume, section 9.13).  Without the cut
        // the mesh is the one-shot's to the bit; the cut, when on, acts
        // within a batch.  0: off, the calls made are the ones above
        int batch_views = 0;
        // > 0 (sparse only): batch_views for the brick-sparse volume.  Three
        // passes with one batch loaded at a time -- the bounds (skipped with
        // use_aabb), the marks, the integration without growth -- into a
        // persistent brick-sparse volume (smvs_tsdf_sparse_volume, section
        // 9.14); cull puts the brick cull in front of the marks.  Without the
        // cut the mesh is the one-shot sparse one to the bit.  0: off, the
        // calls made are the ones above
        int sparse_batch_views = 0;
    };
    TriangleMesh::Ptr generate_fused(std::vector<SceneView> const& views,
        std::string const& image_name, std::string const& dm_name,
        FusedOptions const& fused, smvs_mesh_clean_stats* clean_stats = nullptr);
    // (clean_stats: what the clean counted, with fused.clean)

private:
    struct Inputs;
    // loads the usable views' maps and images into the device's view records
    void load_views(std::vector<SceneView> const& inputviews,
        std::string const& image_name, std::string const& dm_name, Inputs& in) const;
    void save_cut_maps(Inputs const& in) const;
    TriangleMesh::Ptr generate_fused_batched(std::vector<SceneView> const& views,
        std::string const& image_name, std::string const& dm_name,
        FusedOptions const& fused, std::size_t step, FusedBatchVolume& volume,
        smvs_mesh_clean_stats* clean_stats);

    Options opts;
};

// mve::geom::save_ply_mesh with vertex normals, values and confidences
// (binary little endian; x y z nx ny nz red green blue confidence value;
// an empty face element), streamed from the SoA buffers
void save_ply_points(std::string const& path, PointCloud const& points);

// mve::geom::save_ply_mesh of the triangle mesh with smvsrecon's options
// (DESIGN.md M6): x y z nx ny nz red green blue confidence, no value, and
// `element face` as `uchar 3` + three int32 per face; streamed
void save_ply_mesh(std::string const& path, TriangleMesh const& mesh);

// AppSettings of smvsrecon's generate_mesh
struct PointCloudSettings
{
    std::vector<int> view_ids;          // empty: every view of the scene
    std::string image_embedding = "undistorted";
    int input_scale = 0;                // names the embeddings and the file
    bool use_shading = false;
    bool cut_surface = true;            // --no-cut
    bool create_triangle_mesh = false;  // --mesh: generate_scene_mesh; refused
                                        // by generate_scene_point_cloud
    bool simplify = false;              // --simplify: generate_scene_simplified;
                                        // refused by the two entries above
    bool use_aabb = false;
    float aabb_min[3] = { 0, 0, 0 }, aabb_max[3] = { 0, 0, 0 };
    int device = 0;
};

// app/smvsrecon.cc:278-343: generate_mesh over the scene's views, AABB clip,
// <scene>/smvs-{B,S}<input_scale>.ply; -> the file written
std::string generate_scene_point_cloud(std::string const& scene_path,
    PointCloudSettings const& settings, std::size_t* n_points = nullptr);

// the same with --mesh: the triangle mesh, <scene>/smvs-m-{B,S}<input_scale>.ply;
// -> the file written
std::string generate_scene_mesh(std::string const& scene_path,
    PointCloudSettings const& settings, std::size_t* n_vertices = nullptr,
    std::size_t* n_faces = nullptr);

// the same with --simplify (and --mesh when settings.create_triangle_mesh):
// the file names are the reference's, smvs-{B,S}<scale>.ply or
// smvs-m-{B,S}<scale>.ply (--simplify has no name of its own); -> the file
// written.  settings.simplify is implied.
std::string generate_scene_simplified(std::string const& scene_path,
    PointCloudSettings const& settings, std::size_t* n_vertices = nullptr,
    std::size_t* n_faces = nullptr);

// not in the reference: MeshGenerator::generate_fused over the scene's views,
// <scene>/smvs-fused-{B,S}<input_scale>.ply through save_ply_mesh; the box is
// the settings' AABB when use_aabb is set; -> the file written.  With
// fused.clean the cleaned mesh is written instead, as
// <scene>/smvs-clean-{B,S}<input_scale>.ply, and the fused file is not.
std::string generate_scene_fused(std::string const& scene_path,
    PointCloudSettings const& settings, MeshGenerator::FusedOptions const& fused,
    std::size_t* n_vertices = nullptr, std::size_t* n_faces = nullptr,
    smvs_mesh_clean_stats* clean_stats = nullptr);

} // namespace smvs_amd
