// The persistent volume of the volumetric fusion on gfx950 (DESIGN.md section
// 9.13; opt-in): smvs_tsdf_fuse's sums kept on the device between calls, so
// that the views are fused batch by batch.  The normative definition is the
// comment of smvs_tsdf_volume_create in include/smvs_hip.h, restated in numpy
// by tests/tsdf_volume_ref.py.
//
// The volume owns S, W and the colour sums (24 bytes per voxel, the planes and
// the x-fastest order of tsdf.hip); everything else lives in a leased
// workspace for the length of one call:
//   integrate  the batch is prepared as smvs_tsdf_fuse prepares its list (the
//              view stage, tsdf_depth_kernel), then one lane per voxel walks
//              the batch in list order and CONTINUES the stored sums
//   extract    F = S / W into the workspace, then the classify .. fill half of
//              smvs_tsdf_fuse (tsdf_host::extract_surface) on F and the
//              volume's own W and colour planes
// Every call ends with its stream drained: the next call may lease another
// workspace, and with it another stream.
#include "common.h"
#include "mesh_shared.h"
#include "tsdf_shared.h"

#include <cmath>
#include <new>

struct smvs_tsdf_volume {
    int device = 0;
    smvs_tsdf_volume_options options = {};
    smvs_hip::TsdfGrid G = {};     // min_weight and n_views are set per call
    size_t n_vox = 0;
    int64_t n_views = 0;
    float *S = nullptr;
    uint32_t *W = nullptr;
    uint4 *colour = nullptr;
};

namespace smvs_hip {

// Field, steps 1-8 for the views of one batch, from the stored sums.  A block
// is a brick of 8 x 8 x 4 voxels, as in tsdf_integrate_kernel.  The float sum
// S has one order, the view-list order across all batches, so the stored S is
// loaded before the batch's first term is added to it -- at the lane's first
// contributing view, so that a voxel outside every frustum of the batch reads
// nothing -- and the sums are stored only where W changed (S and the colour
// sums change only then).
__global__ void __launch_bounds__(256)
tsdf_volume_integrate_kernel(const MeshViewDev *__restrict__ views,
    const TsdfImageDev *__restrict__ images, TsdfGrid G, float *__restrict__ sum,
    uint32_t *__restrict__ weight, uint4 *__restrict__ colour)
{
#pragma clang fp contract(off)
    int const bricks_x = (G.nx + TSDF_BX - 1) / TSDF_BX;
    int const bricks_y = (G.ny + TSDF_BY - 1) / TSDF_BY;
    int const brick = blockIdx.x;
    int const i = (brick % bricks_x) * TSDF_BX + (threadIdx.x & 7);
    int const j = (brick / bricks_x % bricks_y) * TSDF_BY + (threadIdx.x >> 3 & 7);
    int const k = (brick / bricks_x / bricks_y) * TSDF_BZ + (threadIdx.x >> 6);
    if (i >= G.nx || j >= G.ny || k >= G.nz)
        return;
    float const c[3] = { tsdf_centre(G, 0, i), tsdf_centre(G, 1, j), tsdf_centre(G, 2, k) };
    size_t const at = ((size_t)k * G.ny + j) * G.nx + i;
    float S = 0.0f;
    uint32_t W = 0, R = 0, Gr = 0, B = 0, C = 0;
    bool loaded = false;
    for (int v = 0; v < G.n_views; ++v) {
        MeshViewDev const &V = views[v];
        TSDF_STEPS_1_TO_6(V, c, G.trunc, continue);
        if (!loaded) {
            S = sum[at];
            W = weight[at];
            uint4 const col = colour[at];
            R = col.x;
            Gr = col.y;
            B = col.z;
            C = col.w;
            loaded = true;
        }
        S += fminf(1.0f, sdf / G.trunc);
        W += 1;
        if (sdf <= G.trunc) {
            int const ch = images[v].channels;
            const uint8_t *px = images[v].image + pj * ch;
            uint32_t const g = px[0];
            R += g;
            Gr += ch >= 3 ? px[1] : g;
            B += ch >= 3 ? px[2] : g;
            C += 1;
        }
    }
    if (!loaded)
        return;
    sum[at] = S;
    weight[at] = W;
    colour[at] = make_uint4(R, Gr, B, C);
}

// Extract: F = S / (float)W where W >= min_weight, else NaN
__global__ void __launch_bounds__(256)
tsdf_volume_field_kernel(const float *__restrict__ sum, const uint32_t *__restrict__ weight,
    size_t n_vox, uint32_t min_weight, float *__restrict__ tsdf)
{
#pragma clang fp contract(off)
    size_t const at = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (at >= n_vox)
        return;
    uint32_t const W = weight[at];
    tsdf[at] = W >= min_weight ? sum[at] / (float)W : __builtin_nanf("");
}

} // namespace smvs_hip

using namespace smvs_hip;
using namespace smvs_hip::tsdf_host;

namespace {

int
zero_state(Workspace &ws, smvs_tsdf_volume const &vol)
{
    SMVS_HIP_CHECK(hipMemsetAsync(vol.S, 0, 4 * vol.n_vox, ws.stream));
    SMVS_HIP_CHECK(hipMemsetAsync(vol.W, 0, 4 * vol.n_vox, ws.stream));
    SMVS_HIP_CHECK(hipMemsetAsync(vol.colour, 0, 16 * vol.n_vox, ws.stream));
    SMVS_HIP_CHECK(hipStreamSynchronize(ws.stream));
    return SMVS_OK;
}

void
free_volume(smvs_tsdf_volume *vol)
{
    (void)set_device(vol->device);
    (void)hipFree(vol->S);
    (void)hipFree(vol->W);
    (void)hipFree(vol->colour);
    delete vol;
}

} // namespace

extern "C" int
smvs_tsdf_volume_create(int device, const smvs_tsdf_volume_options *options,
    smvs_tsdf_volume **volume)
{
    SMVS_REQUIRE(volume != nullptr, "no volume pointer");
    *volume = nullptr;
    SMVS_REQUIRE(options != nullptr, "no options");
    TsdfGrid G;
    int rc;
    if ((rc = check_volume_grid("smvs_tsdf_volume_create", *options, 1024, G)))
        return rc;
    size_t const n_vox = (size_t)G.nx * G.ny * G.nz;
    SMVS_REQUIRE(n_vox <= TSDF_MAX_VOXELS, "the volume has more than 2^27 voxels");

    WorkspaceLease lease(device);
    if (lease.w == nullptr)
        return SMVS_ERR_HIP;
    smvs_tsdf_volume *vol = new (std::nothrow) smvs_tsdf_volume();
    if (vol == nullptr) {
        set_error("smvs_tsdf_volume_create: out of host memory");
        return SMVS_ERR_NOMEM;
    }
    vol->device = device;
    vol->options = *options;
    vol->G = G;
    vol->n_vox = n_vox;
    if ((rc = device_malloc(reinterpret_cast<void **>(&vol->S), 4 * n_vox))
        || (rc = device_malloc(reinterpret_cast<void **>(&vol->W), 4 * n_vox))
        || (rc = device_malloc(reinterpret_cast<void **>(&vol->colour), 16 * n_vox))
        || (rc = zero_state(*lease.w, *vol))) {
        free_volume(vol);
        return rc;
    }
    *volume = vol;
    return SMVS_OK;
}

extern "C" int
smvs_tsdf_volume_integrate(smvs_tsdf_volume *volume, const smvs_point_view *views, int n_views,
    int cut_surfaces)
{
    SMVS_REQUIRE(volume != nullptr, "no volume");
    int rc;
    if ((rc = check_views(views, n_views, cut_surfaces, true)))
        return rc;
    SMVS_REQUIRE(volume->n_views + n_views <= VOLUME_MAX_VIEWS,
        "more than 2^24 views in one volume");
    TsdfGrid G = volume->G;
    G.n_views = n_views;

    WorkspaceLease lease(volume->device);
    if (lease.w == nullptr)
        return SMVS_ERR_HIP;
    Workspace &ws = *lease.w;
    ViewStage stage;
    if ((rc = stage(ws, views, n_views, cut_surfaces != 0, true, [](Carver &) {})))
        return rc;
    size_t n_bricks;
    unsigned const bricks = brick_grid(G, &n_bricks).n;
    hipLaunchKernelGGL(tsdf_volume_integrate_kernel, dim3(bricks), dim3(256), 0, ws.stream,
        stage.s.d_table, stage.d_images, G, volume->S, volume->W, volume->colour);
    SMVS_HIP_CHECK(hipGetLastError());
    SMVS_HIP_CHECK(hipStreamSynchronize(ws.stream));
    volume->n_views += n_views;
    return SMVS_OK;
}

extern "C" int
smvs_tsdf_volume_extract(const smvs_tsdf_volume *volume, int min_weight, float *tsdf,
    uint32_t *weight, smvs_points **handle, int64_t *n_vertices, int64_t *n_faces)
{
    SMVS_REQUIRE(handle != nullptr, "no handle pointer");
    *handle = nullptr;
    SMVS_REQUIRE(volume != nullptr, "no volume");
    TsdfGrid G = volume->G;
    G.min_weight = min_weight > 0 ? (uint32_t)min_weight : 1u;
    G.n_views = (int)volume->n_views;
    size_t const n_vox = volume->n_vox;

    WorkspaceLease lease(volume->device);
    if (lease.w == nullptr)
        return SMVS_ERR_HIP;
    Workspace &ws = *lease.w;
    Carver carve;
    size_t const tsdf_at = carve(4 * n_vox);
    ExtractPieces extract_at;
    carve_extract(n_vox, carve, extract_at);
    char *slab = nullptr;
    int rc;
    if ((rc = ws.ensure(0, carve.total, &slab)) != SMVS_OK)
        return rc;
    float *d_tsdf = reinterpret_cast<float *>(slab + tsdf_at);
    hipLaunchKernelGGL(tsdf_volume_field_kernel, dim3(extract_at.point_blocks), dim3(256), 0,
        ws.stream, volume->S, volume->W, n_vox, G.min_weight, d_tsdf);
    smvs_points *h = nullptr;
    if ((rc = extract_surface(ws, "smvs_tsdf_volume_extract", G, slab, extract_at, d_tsdf,
            volume->W, volume->colour, &h)))
        return rc;
    if ((tsdf != nullptr && (rc = ws.download(tsdf, d_tsdf, 4 * n_vox)))
        || (weight != nullptr && (rc = ws.download(weight, volume->W, 4 * n_vox)))) {
        delete h;
        return rc;
    }
    // (fill_points has drained the stream)
    return publish(h, handle, n_vertices, n_faces);
}

extern "C" int
smvs_tsdf_volume_info(const smvs_tsdf_volume *volume, smvs_tsdf_volume_options *options,
    int64_t *n_views, int *device)
{
    SMVS_REQUIRE(volume != nullptr, "no volume");
    if (options != nullptr)
        *options = volume->options;
    if (n_views != nullptr)
        *n_views = volume->n_views;
    if (device != nullptr)
        *device = volume->device;
    return SMVS_OK;
}

extern "C" int
smvs_tsdf_volume_download(const smvs_tsdf_volume *volume, float *S, uint32_t *W, uint32_t *rgbc)
{
    SMVS_REQUIRE(volume != nullptr, "no volume");
    WorkspaceLease lease(volume->device);
    if (lease.w == nullptr)
        return SMVS_ERR_HIP;
    Workspace &ws = *lease.w;
    size_t const n_vox = volume->n_vox;
    int rc;
    if ((S != nullptr && (rc = ws.download(S, volume->S, 4 * n_vox)))
        || (W != nullptr && (rc = ws.download(W, volume->W, 4 * n_vox)))
        || (rgbc != nullptr && (rc = ws.download(rgbc, volume->colour, 16 * n_vox))))
        return rc;
    return SMVS_OK;
}

extern "C" int
smvs_tsdf_volume_upload(smvs_tsdf_volume *volume, const float *S, const uint32_t *W,
    const uint32_t *rgbc, int64_t n_views)
{
    SMVS_REQUIRE(volume != nullptr, "no volume");
    SMVS_REQUIRE(S != nullptr && W != nullptr && rgbc != nullptr, "no state");
    SMVS_REQUIRE(n_views >= 0 && n_views <= VOLUME_MAX_VIEWS, "n_views must be 0 .. 2^24");
    WorkspaceLease lease(volume->device);
    if (lease.w == nullptr)
        return SMVS_ERR_HIP;
    Workspace &ws = *lease.w;
    size_t const n_vox = volume->n_vox;
    int rc;
    if ((rc = ws.upload(volume->S, S, 4 * n_vox)) || (rc = ws.upload(volume->W, W, 4 * n_vox))
        || (rc = ws.upload(volume->colour, rgbc, 16 * n_vox)))
        return rc;
    SMVS_HIP_CHECK(hipStreamSynchronize(ws.stream));
    volume->n_views = n_views;
    return SMVS_OK;
}

extern "C" int
smvs_tsdf_volume_reset(smvs_tsdf_volume *volume)
{
    SMVS_REQUIRE(volume != nullptr, "no volume");
    WorkspaceLease lease(volume->device);
    if (lease.w == nullptr)
        return SMVS_ERR_HIP;
    int rc;
    if ((rc = zero_state(*lease.w, *volume)))
        return rc;
    volume->n_views = 0;
    return SMVS_OK;
}

extern "C" void
smvs_tsdf_volume_release(smvs_tsdf_volume *volume)
{
    if (volume != nullptr)
        free_volume(volume);
}
