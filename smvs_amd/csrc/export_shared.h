// Host side of the scene-export layer, shared by every path that turns depth
// maps into geometry (mesh.hip, simplify.hip, tsdf.hip, tsdf_sparse.hip,
// tsdf_cull.hip): the view stage (mesh_cut.hip), the exclusive scan, the AABB
// vertex clip and the result fill (export_common.hip).  A new export path
// calls these; it does not copy them.
#pragma once

#include "common.h"
#include "mesh_shared.h"

#include <vector>

// the handle every export entry returns (smvs_points_info / _download / _release)
struct smvs_points {
    bool mesh = false;   // smvs_mesh_generate: no values, faces always
    int64_t n_points = 0, n_faces = 0;
    std::vector<float> xyz, nrm, conf, val;
    std::vector<uint8_t> rgb;
    std::vector<uint32_t> faces;
    bool sparse = false;          // smvs_tsdf_fuse_sparse: cells per vertex
    std::vector<int64_t> cells;
};

namespace smvs_hip {

// lays pieces out in a workspace slab, each 256-byte aligned
struct Carver {
    size_t total = 0;
    size_t operator()(size_t bytes)
    {
        size_t const at = total;
        total += (bytes + 255) & ~(size_t)255;
        return at;
    }
};

// ------------------------------------------------------- view stage (mesh_cut.hip)
// The views' maps and camera table in a workspace slab, uploaded, prepared
// (normals to world space, z-depth) and cut.
struct ViewPieces {
    size_t depth_z, depth_ray, cut, normals, image;   // offsets in the slab
};
struct ViewSlab {
    std::vector<ViewPieces> at;    // per view
    size_t table_at = 0, max_pix = 0;
    std::vector<MeshViewDev> table;
    std::vector<const uint8_t *> images;   // per view, on the device (null without images)
    MeshViewDev *d_table = nullptr;
};
// want_images == false: no image is carved or uploaded
void carve_views(const smvs_point_view *views, int n_views, bool want_images, Carver &carve,
    ViewSlab &s);
// uploads the views and the table, then generate_mesh :197-215 for all views:
// normals to world space, and the cut when asked for and there is more than
// one view (:211).  A view without normals gets zeros.
int upload_and_prepare(Workspace &ws, char *slab, const smvs_point_view *views, int n_views,
    bool cut, bool want_images, ViewSlab &s);

// ------------------------------------------------------ scan (export_common.hip)
// exclusive scan of n 64-bit values in place; tiles: (n + SCAN_TILE - 1) /
// SCAN_TILE + 1 words, the grand total behind the last tile
constexpr int SCAN_ITEMS = 16, SCAN_TILE = 256 * SCAN_ITEMS;
int exclusive_scan(hipStream_t stream, unsigned long long *a, size_t n,
    unsigned long long *tiles);
// the word of `tiles` that holds the total of an n-element scan
inline unsigned long long *
scan_total(unsigned long long *tiles, size_t n)
{
    return tiles + (n + SCAN_TILE - 1) / SCAN_TILE;
}

// ------------------------------------------------- AABB clip (export_common.hip)
// the per-vertex arrays of a PointBufs or a SimpOut; val == nullptr: no values
struct VertexAttrs {
    float *xyz, *nrm;
    uint8_t *rgb;
    float *conf, *val;
};
template <class Bufs>
inline VertexAttrs
vertex_attrs(Bufs const &b)
{
    return VertexAttrs{ b.xyz, b.nrm, b.rgb, b.conf, b.val };
}
// smvsrecon.cc:306-319 on n vertices: keep flags into `scan`, their exclusive
// scan (the new ids; the kept count ends up in *scan_total(tiles, n)) and the
// order-preserving compaction src -> dst.  Only enqueues.
int launch_aabb_clip(hipStream_t stream, size_t n, float3 lo, float3 hi, VertexAttrs src,
    VertexAttrs dst, unsigned long long *scan, unsigned long long *tiles);

// ----------------------------------------------- result fill (export_common.hip)
// sizes an smvs_points (mesh, sparse: its flags of the same names) and
// downloads into it, in this order: v's arrays (v.val null: no values), cells
// (the sparse path's cell per vertex, or null), faces (null: none are
// returned); on failure nothing is left behind
int fill_points(Workspace &ws, bool mesh, bool sparse, size_t n_vert, size_t n_face,
    VertexAttrs const &v, const uint32_t *faces, const long long *cells, smvs_points **handle);

} // namespace smvs_hip
