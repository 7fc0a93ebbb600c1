// Device side of what the export paths share (mesh_cut.hip, mesh.hip,
// simplify.hip, the tsdf sources, export_common.hip): the per-view camera
// record, world_point, the AABB test and recalc_normals' face term.  The host
// side (view stage, scan, clip, result fill) is export_shared.h.
#pragma once

#include "common.h"

namespace smvs_hip {

struct MeshViewDev {
    int w, h;
    float invproj[9];   // CameraInfo::fill_inverse_calibration
    float KR[9];        // ViewProjection::KR = K * R
    float t[3];         // ViewProjection::t = KR * camera position
    float rot[9];       // world -> camera rotation
    float c2w_t[3];     // translation column of the cam-to-world matrix
    float *depth_z;     // depthmaps[i] after depthmap_convert_conventions(false)
    float *depth_ray;   // cutmaps_j[i]: the input ray-length depth
    float *cut;         // cutmaps[i]
    float *normals;     // world space after the preparation pass
};

__device__ __forceinline__ float
dot3(const float *a, const float *b)
{
#pragma clang fp contract(off)
    float s = 0.0f;
    s += a[0] * b[0];
    s += a[1] * b[1];
    s += a[2] * b[2];
    return s;
}

// mve::geom::pixel_3dpos followed by Matrix4f::mult(pos, 1) with the
// cam-to-world matrix (mesh_generator.cc:80-82, 120-123)
__device__ __forceinline__ void
world_point(MeshViewDev const &V, int x, int y, float depth, float *pos)
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
    float const len = sqrtf(dot3(v, v));
    float pc[3];
    for (int r = 0; r < 3; ++r)
        pc[r] = v[r] / len * depth;
    for (int r = 0; r < 3; ++r) {
        float s = 0.0f;
        s += V.rot[r] * pc[0];
        s += V.rot[3 + r] * pc[1];
        s += V.rot[6 + r] * pc[2];
        pos[r] = s + V.c2w_t[r] * 1.0f;
    }
}

// smvsrecon.cc:310-315: any coordinate below the minimum or above the maximum
__device__ __forceinline__ bool
outside_aabb(const float *q, float3 lo, float3 hi)
{
    return q[0] < lo.x || q[0] > hi.x || q[1] < lo.y || q[1] > hi.y
        || q[2] < lo.z || q[2] > hi.z;
}

// M3 / M4 for face (a, b, c) = q[0..2]: the unit face normal and the angle at
// corner k; -> false for a face of zero area (it adds nothing)
__device__ __forceinline__ bool
face_term(const float (*q)[3], int k, float *fn, float *weight)
{
#pragma clang fp contract(off)
    float ab[3], bc[3], ca[3], nca[3];
    for (int r = 0; r < 3; ++r) {
        ab[r] = q[1][r] - q[0][r];
        bc[r] = q[2][r] - q[1][r];
        ca[r] = q[0][r] - q[2][r];
        nca[r] = -ca[r];
    }
    fn[0] = ab[1] * nca[2] - ab[2] * nca[1];
    fn[1] = ab[2] * nca[0] - ab[0] * nca[2];
    fn[2] = ab[0] * nca[1] - ab[1] * nca[0];
    float const fnl = sqrtf(dot3(fn, fn));
    if (fnl == 0.0f)
        return false;
    for (int r = 0; r < 3; ++r)
        fn[r] = fn[r] / fnl;
    float const lab = sqrtf(dot3(ab, ab)), lbc = sqrtf(dot3(bc, bc)),
        lca = sqrtf(dot3(ca, ca));
    float cosine;
    if (k == 0) {
        cosine = dot3(ab, nca) / (lab * lca);
    } else if (k == 1) {
        float const nab[3] = { -ab[0], -ab[1], -ab[2] };
        cosine = dot3(nab, bc) / (lab * lbc);
    } else {
        float const nbc[3] = { -bc[0], -bc[1], -bc[2] };
        cosine = dot3(ca, nbc) / (lca * lbc);
    }
    cosine = cosine < -1.0f ? -1.0f : (cosine > 1.0f ? 1.0f : cosine);
    *weight = acosf(cosine);
    return true;
}

} // namespace smvs_hip
