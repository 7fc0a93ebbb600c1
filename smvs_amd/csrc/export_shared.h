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
// Vertex i of src becomes vertex j of dst, bit for bit: what an
// order-preserving compaction does once its keep flag has spoken (the AABB
// clip and the mesh clean differ in the flag alone).  A macro and not a
// function: expanded in the clip's kernel it leaves that kernel the instruction
// stream it had (an inlined function reorders its address arithmetic).
#define SMVS_COPY_VERTEX(src, i, dst, j)                                      \
    do {                                                                      \
        for (int r = 0; r < 3; ++r) {                                         \
            (dst).xyz[3 * (j) + r] = (src).xyz[3 * (i) + r];                  \
            (dst).nrm[3 * (j) + r] = (src).nrm[3 * (i) + r];                  \
            (dst).rgb[3 * (j) + r] = (src).rgb[3 * (i) + r];                  \
        }                                                                     \
        (dst).conf[j] = (src).conf[i];                                        \
        if ((dst).val != nullptr) /* (a triangle mesh has no values) */       \
            (dst).val[j] = (src).val[i];                                      \
    } while (0)
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

// ------------------------------------------------------ mesh clean (mesh_clean.hip)
// smvs_mesh_clean's definition (include/smvs_hip.h) from device arrays to device
// arrays.  Only enqueues: a fusion entry can call it on its vertices and faces
// before fill_points, with no host round trip in between.
struct MeshCleanCounts {   // on the device; what the stats and the handle's sizes are read from
    float cut_value;
    uint32_t pad;
    unsigned long long n_cut, n_components, n_small_components, n_small_vertices,
        n_unreferenced, largest_component, n_vertices, n_faces;
};
struct MeshCleanWork {     // pieces of a workspace slab, see carve_mesh_clean
    MeshCleanCounts *counts;
    uint32_t *select;                  // the radix select's state and histogram
    uint32_t *label, *count, *size;    // per vertex; size == nullptr: not wanted
    uint8_t *cut, *referenced, *survive;   // per vertex, per vertex, per face
    unsigned long long *vscan, *vtiles, *fscan, *ftiles;
};
// lays the work arrays of n vertices and m faces out in a slab; resolve with
// mesh_clean_work once the slab exists
struct MeshCleanPieces {
    size_t counts, select, label, count, size, cut, referenced, survive, vscan, vtiles, fscan,
        ftiles;
    bool want_size;
};
MeshCleanPieces carve_mesh_clean(Carver &carve, size_t n, size_t m, bool want_size);
MeshCleanWork mesh_clean_work(char *slab, MeshCleanPieces const &at);
// src (n vertices, cells may be null, m faces) -> dst, arrays with room for n
// vertices and m faces.  Afterwards, on the stream: work.counts filled;
// work.label = `component`, work.size = `component_size` (when wanted) and
// work.vscan = `new_id` (as int64) of the definition.
int launch_mesh_clean(hipStream_t stream, size_t n, size_t m, VertexAttrs src,
    const long long *src_cells, const uint32_t *src_faces, smvs_mesh_clean_options const &opt,
    MeshCleanWork const &work, VertexAttrs dst, long long *dst_cells, uint32_t *dst_faces);

} // namespace smvs_hip
