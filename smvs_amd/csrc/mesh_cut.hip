// Cross-view consistency cut of the depth maps on gfx950.
//
// Replaces MeshGenerator::cut_depth_maps (reference: lib/mesh_generator.cc:24-158)
// together with the normal preparation of generate_mesh (:189-208) and
// MeshGenerator::ViewProjection (:300-342).  Every pixel of every view is an
// independent unit: its 3-D point is reprojected into all other views and
// kept when enough of them see a compatible surface there.  One thread per
// pixel walks the other views in the reference's order (the consistency sum
// and its early exit are order dependent); all maps stay resident on the
// device, so N views cost one upload and one download of N maps.
//
// Arithmetic: float, in the reference's operation order, FMA contraction off
// (hipcc's float division and square root are correctly rounded), so the cut
// maps are bit-identical to the CPU path.  MVE pieces (pixel_3dpos,
// fill_cam_to_world, fill_camera_pos, depthmap_convert_conventions) follow the
// assumptions listed in tests/golden/README.md [MVE-unverified].
//
// The host side below is the view stage every export path starts with
// (export_shared.h): the views' maps carved from a workspace slab, the camera
// table, the uploads and the prepare / cut launches.
#include "common.h"
#include "export_shared.h"
#include "mesh_shared.h"

#include <vector>

namespace smvs_hip {

// ViewProjection::get_surface_power, mesh_generator.cc:321-342
__device__ __forceinline__ float
surface_power(MeshViewDev const &V, const float *pos, const float *normal)
{
#pragma clang fp contract(off)
    const float *KR = V.KR;
    float const u = dot3(KR + 0, pos) - V.t[0];
    float const v = dot3(KR + 3, pos) - V.t[1];
    float const w = dot3(KR + 6, pos) - V.t[2];
    float const denom = w * w;
    float u_dx[3], v_dx[3];
    for (int k = 0; k < 3; ++k) {
        u_dx[k] = (KR[k] * w - KR[6 + k] * u) / denom;
        v_dx[k] = (KR[3 + k] * w - KR[6 + k] * v) / denom;
    }
    float cr[3];
    cr[0] = u_dx[1] * v_dx[2] - u_dx[2] * v_dx[1];
    cr[1] = u_dx[2] * v_dx[0] - u_dx[0] * v_dx[2];
    cr[2] = u_dx[0] * v_dx[1] - u_dx[1] * v_dx[0];
    return -dot3(normal, cr);
}

// generate_mesh :197-208 (normals to world space) and cut_depth_maps :31-47
// (ray-length copies, z-depth conversion) for one view
__global__ void __launch_bounds__(256)
mesh_prepare_kernel(const MeshViewDev *views, int i)
{
#pragma clang fp contract(off)
    MeshViewDev const V = views[i];
    int const x = blockIdx.x * blockDim.x + threadIdx.x;
    int const y = blockIdx.y;
    if (x >= V.w)
        return;
    size_t const p = (size_t)y * V.w + x;
    float const n[3] = { V.normals[3 * p], -V.normals[3 * p + 1],
        -V.normals[3 * p + 2] };
    for (int r = 0; r < 3; ++r) {
        float s = 0.0f;
        s += V.rot[r] * n[0];
        s += V.rot[3 + r] * n[1];
        s += V.rot[6 + r] * n[2];
        V.normals[3 * p + r] = s;
    }
    float const d = V.depth_ray[p];
    V.cut[p] = d;
    float const px = (float)x + 0.5f, py = (float)y + 0.5f;
    float v[3];
    for (int r = 0; r < 3; ++r)
        v[r] = V.invproj[3 * r] * px + V.invproj[3 * r + 1] * py
            + V.invproj[3 * r + 2];
    float const len = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    // (depthmap_convert_conventions: `double len = px.norm(); dm *= 1.0 / len`,
    // tests/golden/README.md M10)
    V.depth_z[p] = (float)((double)d * (1.0 / (double)len));
}

// cut_depth_maps :61-150 for view i
__global__ void __launch_bounds__(256)
mesh_cut_kernel(const MeshViewDev *__restrict__ views, int n_views, int i)
{
#pragma clang fp contract(off)
    MeshViewDev const V = views[i];
    int const x = blockIdx.x * blockDim.x + threadIdx.x;
    int const y = blockIdx.y;
    if (x >= V.w)
        return;
    size_t const p = (size_t)y * V.w + x;
    float const d = V.depth_ray[p];
    if (d == 0.0f)
        return;
    float pos[3];
    world_point(V, x, y, d, pos);
    float const normal[3] = { V.normals[3 * p], V.normals[3 * p + 1],
        V.normals[3 * p + 2] };
    float const power = surface_power(V, pos, normal);
    bool cut = power < 0;
    float consistency = 0;
    for (int j = 0; j < n_views; ++j) {
        if (j == i)
            continue;
        MeshViewDev const &N = views[j];
        float proj[3];
        proj[0] = dot3(N.KR + 0, pos) - N.t[0];
        proj[1] = dot3(N.KR + 3, pos) - N.t[1];
        proj[2] = dot3(N.KR + 6, pos) - N.t[2];
        if (proj[2] < 0)
            continue;
        // A point in view j's principal plane (proj[2] == 0, or NaN): the
        // reference's quotient is infinite or NaN, its static_cast<int> gives
        // INT_MIN on x86 and the pair is skipped.  A saturating conversion
        // would turn NaN into column 0.
        if (!(proj[2] > 0))
            continue;
        // (int) truncates toward zero, so a quotient in (-1, 0) is column or
        // row 0; the range is tested on the float, and only a finite quotient
        // inside it is converted
        float const qx = proj[0] / proj[2], qy = proj[1] / proj[2];
        if (!(qx > -1.0f && qx < (float)N.w && qy > -1.0f && qy < (float)N.h))
            continue;
        int const xj = (int)qx, yj = (int)qy;
        size_t const pj = (size_t)yj * N.w + xj;
        float const dm_j = N.depth_z[pj];
        if (dm_j == 0.0f)
            continue;
        float const power_j = surface_power(N, pos, normal);
        float pos_j[3];
        world_point(N, xj, yj, N.depth_ray[pj], pos_j);
        float const normal_j[3] = { N.normals[3 * pj], N.normals[3 * pj + 1],
            N.normals[3 * pj + 2] };
        float const power_j_j = surface_power(N, pos_j, normal_j);
        if ((double)dm_j * 1.01 < (double)proj[2])
            continue;
        if ((double)dm_j * 0.997 > (double)proj[2]) {
            if ((double)power_j_j > 0.5 * (double)power)
                consistency -= power_j_j;
            continue;
        }
        if ((double)power_j_j > 2.0 * (double)power
            || (double)power_j > 2.0 * (double)power) {
            cut = true;
            break;
        }
        consistency += power_j_j;
    }
    if (consistency <= 0)
        cut = true;
    if (cut)
        V.cut[p] = 0.0f;
}

static void
mat3_mul_f(const float *A, const float *B, float *C)
{
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            float s = 0.0f;
            for (int k = 0; k < 3; ++k)
                s += A[3 * r + k] * B[3 * k + c];
            C[3 * r + c] = s;
        }
}

// CameraInfo::fill_calibration / fill_inverse_calibration (ppoint = 0.5,
// paspect = 1) at the depth map's size, ViewProjection's KR and t, and the
// cam-to-world transform of one view
static void
fill_view_camera(int width, int height, float flen, const float *rot,
    const float *trans, MeshViewDev &V)
{
    V.w = width;
    V.h = height;
    float const fw = (float)width, fh = (float)height;
    float const dim = fw > fh ? fw : fh;
    float const ax = flen * dim, ay = flen * dim;
    float const K[9] = { ax, 0, fw * 0.5f, 0, ay, fh * 0.5f, 0, 0, 1 };
    float const Ki[9] = { 1.0f / ax, 0, -fw * 0.5f / ax, 0, 1.0f / ay,
        -fh * 0.5f / ay, 0, 0, 1 };
    memcpy(V.invproj, Ki, sizeof(Ki));
    memcpy(V.rot, rot, sizeof(V.rot));
    mat3_mul_f(K, rot, V.KR);
    // fill_camera_pos = fill_cam_to_world's translation = -R^T t
    float pos[3];
    for (int r = 0; r < 3; ++r) {
        float s = 0.0f;
        for (int k = 0; k < 3; ++k)
            s += -rot[3 * k + r] * trans[k];
        pos[r] = s;
        V.c2w_t[r] = s;
    }
    for (int r = 0; r < 3; ++r) {
        float s = 0.0f;
        for (int k = 0; k < 3; ++k)
            s += V.KR[3 * r + k] * pos[k];
        V.t[r] = s;
    }
}

// generate_mesh :197-215 for all views: normals to world space, then the cut
// when asked for and there is more than one view (:211)
static int
launch_prepare_and_cut(hipStream_t stream, const MeshViewDev *d_table,
    std::vector<MeshViewDev> const &table, bool cut)
{
    int const n_views = (int)table.size();
    for (int i = 0; i < n_views; ++i)
        hipLaunchKernelGGL(mesh_prepare_kernel,
            dim3((table[i].w + 255) / 256, table[i].h), dim3(256), 0, stream,
            d_table, i);
    SMVS_HIP_CHECK(hipGetLastError());
    if (cut && n_views > 1)
        for (int i = 0; i < n_views; ++i)
            hipLaunchKernelGGL(mesh_cut_kernel,
                dim3((table[i].w + 255) / 256, table[i].h), dim3(256), 0, stream,
                d_table, n_views, i);
    SMVS_HIP_CHECK(hipGetLastError());
    return SMVS_OK;
}

void
carve_views(const smvs_point_view *views, int n_views, bool want_images, Carver &carve,
    ViewSlab &s)
{
    s.at.resize(n_views);
    for (int i = 0; i < n_views; ++i) {
        size_t const npix = (size_t)views[i].width * views[i].height;
        s.max_pix = npix > s.max_pix ? npix : s.max_pix;
        ViewPieces &at = s.at[i];
        at.depth_z = carve(sizeof(float) * npix);
        at.depth_ray = carve(sizeof(float) * npix);
        at.cut = carve(sizeof(float) * npix);
        at.normals = carve(sizeof(float) * 3 * npix);
        at.image = want_images ? carve(npix * views[i].channels) : 0;
    }
    s.table_at = carve(sizeof(MeshViewDev) * n_views);
}

int
upload_and_prepare(Workspace &ws, char *slab, const smvs_point_view *views, int n_views,
    bool cut, bool want_images, ViewSlab &s)
{
    int rc;
    s.table.resize(n_views);
    s.images.assign(n_views, nullptr);
    for (int i = 0; i < n_views; ++i) {
        smvs_point_view const &in = views[i];
        MeshViewDev &V = s.table[i];
        fill_view_camera(in.width, in.height, in.flen, in.rot, in.trans, V);
        size_t const npix = (size_t)in.width * in.height;
        ViewPieces const &at = s.at[i];
        V.depth_z = reinterpret_cast<float *>(slab + at.depth_z);
        V.depth_ray = reinterpret_cast<float *>(slab + at.depth_ray);
        V.cut = reinterpret_cast<float *>(slab + at.cut);
        V.normals = reinterpret_cast<float *>(slab + at.normals);
        if ((rc = ws.upload(V.depth_ray, in.depth, sizeof(float) * npix)))
            return rc;
        // without normals (cut off only) the preparation turns zeros
        if (in.normals != nullptr) {
            if ((rc = ws.upload(V.normals, in.normals, sizeof(float) * 3 * npix)))
                return rc;
        } else
            SMVS_HIP_CHECK(hipMemsetAsync(V.normals, 0, sizeof(float) * 3 * npix,
                ws.stream));
        if (want_images) {
            uint8_t *img = reinterpret_cast<uint8_t *>(slab + at.image);
            s.images[i] = img;
            if ((rc = ws.upload(img, in.image, npix * in.channels)))
                return rc;
        }
    }
    s.d_table = reinterpret_cast<MeshViewDev *>(slab + s.table_at);
    if ((rc = ws.upload(s.d_table, s.table.data(), sizeof(MeshViewDev) * n_views)))
        return rc;
    return launch_prepare_and_cut(ws.stream, s.d_table, s.table, cut);
}

} // namespace smvs_hip

using namespace smvs_hip;

extern "C" int
smvs_cut_depth_maps(int device, smvs_mesh_view *views, int n_views)
{
    SMVS_REQUIRE(views != nullptr && n_views >= 1, "no views");
    SMVS_REQUIRE(n_views <= 4096, "too many views");
    for (int i = 0; i < n_views; ++i)
        SMVS_REQUIRE(views[i].width > 0 && views[i].height > 0
            && views[i].depth != nullptr && views[i].normals != nullptr
            && views[i].flen > 0.0f, "bad view");
    // the view stage takes point views: these carry no image
    std::vector<smvs_point_view> pviews(n_views);
    for (int i = 0; i < n_views; ++i) {
        smvs_mesh_view const &in = views[i];
        smvs_point_view &P = pviews[i];
        P = smvs_point_view();
        P.width = in.width;
        P.height = in.height;
        P.flen = in.flen;
        memcpy(P.rot, in.rot, sizeof(P.rot));
        memcpy(P.trans, in.trans, sizeof(P.trans));
        P.depth = in.depth;
        P.normals = in.normals;
    }
    // one slab of a pooled workspace (pool.hip) holds every view's maps and
    // the view table: no allocation per call
    WorkspaceLease lease(device);
    if (lease.w == nullptr)
        return SMVS_ERR_HIP;
    Workspace &ws = *lease.w;
    Carver carve;
    ViewSlab s;
    carve_views(pviews.data(), n_views, false, carve, s);
    char *slab = nullptr;
    int rc;
    if ((rc = ws.ensure(0, carve.total, &slab)) != SMVS_OK)
        return rc;
    // a single depth map is returned unchanged (mesh_generator.cc:211)
    if ((rc = upload_and_prepare(ws, slab, pviews.data(), n_views, true, false, s)))
        return rc;
    for (int i = 0; i < n_views; ++i) {
        size_t const npix = (size_t)s.table[i].w * s.table[i].h;
        if ((rc = ws.download(views[i].depth, s.table[i].cut, sizeof(float) * npix))
            || (rc = ws.download(views[i].normals, s.table[i].normals,
                    sizeof(float) * 3 * npix)))
            return rc;
    }
    return SMVS_OK;
}
