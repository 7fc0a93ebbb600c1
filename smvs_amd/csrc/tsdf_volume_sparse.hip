// The persistent brick-sparse volume of the volumetric fusion on gfx950
// (opt-in): smvs_tsdf_fuse_sparse's sums kept on the
// device between calls, so that grids of up to 4096 voxels per side are fused
// batch by batch.  The normative definition is the comment of
// smvs_tsdf_sparse_volume_create in include/smvs_hip.h, restated in numpy by
// tests/tsdf_sparse_volume_ref.py.
//
// The volume owns one seed byte per brick of the grid, the table brick -> slot,
// the list slot -> brick (always in linear brick order), birth per slot and S,
// W and the colour sums slot-major (24 bytes per voxel, 6144 per slot);
// everything else lives in a leased workspace for the length of one call:
//   mark       the list's seed bytes by tsdf_sparse.hip's seed pass (with the
//              cull of tsdf_cull.hip in front when asked for), OR-ed with the
//              stored bytes in the workspace; the dilation of the result is
//              counted (tsdf_sparse_dilate_kernel, the scan) and only then are
//              the bytes copied over the stored ones
//   re-slot    where the dilation has bricks without a slot: the table of the
//              dilation (tsdf_sparse_table_kernel), new planes, and one block
//              per new slot that copies the brick's 256 x 24 bytes from its
//              old slot or stores zeros.  Old and new planes exist side by side
//              for this one step (the peak: 6144 bytes times old + new slots);
//              the old ones are freed before the integration launches
//   integrate  one block per slot walks the batch in list order and CONTINUES
//              the stored sums, as tsdf_volume_integrate_kernel does
//   extract    F = S / W slot-major into the workspace, then the classify ..
//              fill half of smvs_tsdf_fuse_sparse (tsdf_host::
//              extract_sparse_surface) on F and the volume's own planes
// Arithmetic: float, FMA contraction off.  No atomics: every order is an index
// order.  Every call ends with its stream drained.
#include "common.h"
#include "mesh_shared.h"
#include "tsdf_shared.h"

#include <cmath>
#include <cstring>
#include <new>
#include <vector>

struct smvs_tsdf_sparse_volume {
    int device = 0;
    smvs_tsdf_sparse_volume_options options = {};
    smvs_hip::TsdfGrid G = {};     // min_weight and n_views are set per call
    smvs_hip::TsdfBricks B = {};
    size_t n_bricks = 0;
    int64_t max_bricks = 0;
    int64_t n_views = 0;
    // what the host knows of the device state
    size_t n_seeds = 0, n_dilated = 0, n_slots = 0, n_late = 0;
    uint8_t *seed = nullptr;       // per brick: 2 or 0
    int32_t *table = nullptr;      // per brick: slot or -1
    uint32_t *list = nullptr;      // per slot
    uint32_t *birth = nullptr;     // per slot
    float *S = nullptr;            // per slot 256
    uint32_t *W = nullptr;
    uint4 *colour = nullptr;
};

namespace smvs_hip {

// Seed merge: batch |= stored, four bricks per lane (both arrays are padded to
// a multiple of four bytes; a seed byte is 2 or 0)
__global__ void __launch_bounds__(256)
tsdf_sparse_volume_merge_kernel(const uint32_t *__restrict__ stored, size_t n_words,
    uint32_t *__restrict__ batch)
{
    size_t const at = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= n_words)
        return;
    batch[at] |= stored[at];
}

// Re-slot: block `slot` of the new planes takes its brick's sums from the old
// slot, or zeros and birth = the stored view count
__global__ void __launch_bounds__(256)
tsdf_sparse_volume_reslot_kernel(const uint32_t *__restrict__ list,
    const int32_t *__restrict__ old_table, const float *__restrict__ old_sum,
    const uint32_t *__restrict__ old_weight, const uint4 *__restrict__ old_colour,
    const uint32_t *__restrict__ old_birth, uint32_t n_views, float *__restrict__ sum,
    uint32_t *__restrict__ weight, uint4 *__restrict__ colour, uint32_t *__restrict__ birth)
{
    int32_t const old = old_table[list[blockIdx.x]];
    size_t const at = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (old >= 0) {
        size_t const from = (size_t)old * 256 + threadIdx.x;
        sum[at] = old_sum[from];
        weight[at] = old_weight[from];
        colour[at] = old_colour[from];
    } else {
        sum[at] = 0.0f;
        weight[at] = 0;
        colour[at] = make_uint4(0, 0, 0, 0);
    }
    if (threadIdx.x == 0)
        birth[blockIdx.x] = old >= 0 ? old_birth[old] : n_views;
}

// upload: the table of a list (the table is all -1 before)
__global__ void __launch_bounds__(256)
tsdf_sparse_volume_scatter_kernel(const uint32_t *__restrict__ list, size_t n_slots,
    int32_t *__restrict__ table)
{
    size_t const slot = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (slot < n_slots)
        table[list[slot]] = (int32_t)slot;
}

// Field, steps 1-8 for the views of one batch, from the stored sums of the
// brick of slot blockIdx.x: tsdf_volume_integrate_kernel on slot-major
// addresses.  The stored sums are loaded at the lane's first contributing view
// and stored only where W changed; a lane outside the grid (a partial brick at
// a high face) touches no memory.
__global__ void __launch_bounds__(256)
tsdf_sparse_volume_integrate_kernel(const MeshViewDev *__restrict__ views,
    const TsdfImageDev *__restrict__ images, TsdfGrid G, TsdfBricks B,
    const uint32_t *__restrict__ list, float *__restrict__ sum, uint32_t *__restrict__ weight,
    uint4 *__restrict__ colour)
{
#pragma clang fp contract(off)
    BrickVoxel const p = brick_voxel(G, B, list[blockIdx.x]);
    if (!p.in_grid)
        return;
    float const c[3] = { tsdf_centre(G, 0, p.i), tsdf_centre(G, 1, p.j), tsdf_centre(G, 2, p.k) };
    size_t const at = (size_t)blockIdx.x * 256 + threadIdx.x;
    float S = 0.0f;
    uint32_t W = 0, R = 0, Gr = 0, Bl = 0, C = 0;
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
            Bl = col.z;
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
            Bl += ch >= 3 ? px[2] : g;
            C += 1;
        }
    }
    if (!loaded)
        return;
    sum[at] = S;
    weight[at] = W;
    colour[at] = make_uint4(R, Gr, Bl, C);
}

// Extract: F = S / (float)W where W >= min_weight, else NaN, slot-major (the
// lanes outside the grid hold W == 0)
__global__ void __launch_bounds__(256)
tsdf_sparse_volume_field_kernel(const float *__restrict__ sum,
    const uint32_t *__restrict__ weight, uint32_t min_weight, float *__restrict__ tsdf)
{
#pragma clang fp contract(off)
    size_t const at = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t const W = weight[at];
    tsdf[at] = W >= min_weight ? sum[at] / (float)W : __builtin_nanf("");
}

} // namespace smvs_hip

using namespace smvs_hip;
using namespace smvs_hip::tsdf_host;

namespace {

// the planes of n slots
struct Planes {
    uint32_t *list = nullptr, *birth = nullptr;
    float *S = nullptr;
    uint32_t *W = nullptr;
    uint4 *colour = nullptr;
};

void
free_planes(Planes &p)
{
    (void)hipFree(p.list);
    (void)hipFree(p.birth);
    (void)hipFree(p.S);
    (void)hipFree(p.W);
    (void)hipFree(p.colour);
    p = Planes();
}

int
alloc_planes(size_t n_slots, Planes &p)
{
    int rc;
    if ((rc = device_malloc(reinterpret_cast<void **>(&p.list), 4 * n_slots))
        || (rc = device_malloc(reinterpret_cast<void **>(&p.birth), 4 * n_slots))
        || (rc = device_malloc(reinterpret_cast<void **>(&p.S), 4 * 256 * n_slots))
        || (rc = device_malloc(reinterpret_cast<void **>(&p.W), 4 * 256 * n_slots))
        || (rc = device_malloc(reinterpret_cast<void **>(&p.colour), 16 * 256 * n_slots))) {
        free_planes(p);
        return rc;
    }
    return SMVS_OK;
}

Planes
planes_of(smvs_tsdf_sparse_volume const &vol)
{
    Planes p;
    p.list = vol.list;
    p.birth = vol.birth;
    p.S = vol.S;
    p.W = vol.W;
    p.colour = vol.colour;
    return p;
}

// the volume takes the planes; its old ones are freed
void
adopt_planes(smvs_tsdf_sparse_volume &vol, Planes const &p, size_t n_slots)
{
    Planes old = planes_of(vol);
    free_planes(old);
    vol.list = p.list;
    vol.birth = p.birth;
    vol.S = p.S;
    vol.W = p.W;
    vol.colour = p.colour;
    vol.n_slots = n_slots;
}

size_t
padded(size_t n_bricks)
{
    return (n_bricks + 255) & ~(size_t)255;
}

// seeds, table and the host's counts to "nothing marked"; the planes are freed
int
empty_state(Workspace &ws, smvs_tsdf_sparse_volume &vol)
{
    SMVS_HIP_CHECK(hipMemsetAsync(vol.seed, 0, padded(vol.n_bricks), ws.stream));
    SMVS_HIP_CHECK(hipMemsetAsync(vol.table, 0xff, 4 * vol.n_bricks, ws.stream));
    SMVS_HIP_CHECK(hipStreamSynchronize(ws.stream));
    adopt_planes(vol, Planes(), 0);
    vol.n_seeds = vol.n_dilated = vol.n_late = 0;
    vol.n_views = 0;
    return SMVS_OK;
}

void
free_volume(smvs_tsdf_sparse_volume *vol)
{
    (void)set_device(vol->device);
    Planes p = planes_of(*vol);
    free_planes(p);
    (void)hipFree(vol->seed);
    (void)hipFree(vol->table);
    delete vol;
}

int
over_budget(const char *who, size_t need, int64_t max_bricks)
{
    set_error("%s: the surface needs %lld bricks (%lld bytes of state), max_bricks is %lld", who,
        (long long)need, (long long)need * (long long)VOLUME_STATE_BYTES_PER_BRICK,
        (long long)max_bricks);
    return SMVS_ERR_NOMEM;
}

// mark and integrate.  mark: the list's seeds are OR-ed into the stored ones;
// integrate: the bricks of the dilation get their slots and the list is summed.
// The budget is checked, and the new planes exist, before anything is committed.
int
run(const char *who, smvs_tsdf_sparse_volume &vol, const smvs_point_view *views, int n_views,
    bool cut, bool cull, bool mark, bool integrate)
{
    TsdfGrid G = vol.G;
    G.n_views = n_views;
    TsdfBricks const B = vol.B;
    size_t const n_bricks = vol.n_bricks;
    int rc;

    WorkspaceLease lease(vol.device);
    if (lease.w == nullptr)
        return SMVS_ERR_HIP;
    Workspace &ws = *lease.w;
    hipStream_t const stream = ws.stream;
    // (the table's place holds the cull's candidate list first, as in the one-shot entry)
    ViewStage stage;
    BrickWork w;
    if ((rc = stage(ws, views, n_views, cut, integrate,
            [&](Carver &carve) { w.carve(views, n_views, n_bricks, mark && cull, carve); })))
        return rc;
    ViewSlab const &s = stage.s;
    w.place(stage.slab);

    // the would-be seeds, their dilation and its count
    const uint8_t *d_seeds_now = vol.seed;
    size_t n_seeds = vol.n_seeds, n_dilated = vol.n_dilated;
    if (mark) {
        size_t n_tested;
        if ((rc = launch_seeds(ws, stage.slab, s, n_views, G, B, w, nullptr, &n_tested)))
            return rc;
        size_t const n_words = (n_bricks + 3) / 4;
        hipLaunchKernelGGL(tsdf_sparse_volume_merge_kernel, dim3((unsigned)((n_words + 255) / 256)),
            dim3(256), 0, stream, reinterpret_cast<const uint32_t *>(vol.seed), n_words,
            reinterpret_cast<uint32_t *>(w.seed));
        d_seeds_now = w.seed;
    }
    bool const reslot_may_be_needed = integrate && (mark || vol.n_dilated > vol.n_slots);
    if (mark || reslot_may_be_needed) {
        launch_dilate(stream, d_seeds_now, B, w.state, w.counts);
        SMVS_HIP_CHECK(hipGetLastError());
        if ((rc = exclusive_scan(stream, w.counts, w.blocks, w.tiles)))
            return rc;
        unsigned long long sums = 0;
        if ((rc = ws.download(&sums, scan_total(w.tiles, w.blocks), sizeof(sums))))
            return rc;
        n_dilated = (size_t)(sums & 0xffffffffull);
        n_seeds = (size_t)(sums >> 32);
    }
    if ((int64_t)n_dilated > vol.max_bricks)
        return over_budget(who, n_dilated, vol.max_bricks);

    // Re-slot.  Slots are a subset of the dilation, so equal counts are equal sets.
    if (integrate && n_dilated > vol.n_slots) {
        Planes fresh;
        if ((rc = alloc_planes(n_dilated, fresh)))
            return rc;
        launch_table(stream, w.state, B, w.counts, w.table, fresh.list);
        hipLaunchKernelGGL(tsdf_sparse_volume_reslot_kernel, dim3((unsigned)n_dilated), dim3(256),
            0, stream, fresh.list, vol.table, vol.S, vol.W, vol.colour, vol.birth,
            (uint32_t)vol.n_views, fresh.S, fresh.W, fresh.colour, fresh.birth);
        hipError_t err = hipGetLastError();
        if (err == hipSuccess)
            err = hipStreamSynchronize(stream);
        // (the old table was read to the end: the new one takes its place)
        if (err == hipSuccess)
            err = hipMemcpyAsync(vol.table, w.table, 4 * n_bricks, hipMemcpyDeviceToDevice, stream);
        if (err == hipSuccess)
            err = hipStreamSynchronize(stream);
        if (err != hipSuccess) {
            free_planes(fresh);
            set_error("%s: re-slot failed: %s", who, hipGetErrorString(err));
            return SMVS_ERR_HIP;
        }
        if (vol.n_views > 0)
            vol.n_late += n_dilated - vol.n_slots;
        adopt_planes(vol, fresh, n_dilated);      // frees the old planes
    }
    if (mark) {
        SMVS_HIP_CHECK(hipMemcpyAsync(vol.seed, w.seed, n_bricks, hipMemcpyDeviceToDevice, stream));
        vol.n_seeds = n_seeds;
        vol.n_dilated = n_dilated;
    }
    if (integrate && vol.n_slots > 0) {
        hipLaunchKernelGGL(tsdf_sparse_volume_integrate_kernel, dim3((unsigned)vol.n_slots),
            dim3(256), 0, stream, s.d_table, stage.d_images, G, B, vol.list, vol.S, vol.W,
            vol.colour);
        SMVS_HIP_CHECK(hipGetLastError());
    }
    SMVS_HIP_CHECK(hipStreamSynchronize(stream));
    if (integrate)
        vol.n_views += n_views;
    return SMVS_OK;
}

} // namespace

extern "C" int
smvs_tsdf_sparse_volume_create(int device, const smvs_tsdf_sparse_volume_options *options,
    smvs_tsdf_sparse_volume **volume)
{
    SMVS_REQUIRE(volume != nullptr, "no volume pointer");
    *volume = nullptr;
    SMVS_REQUIRE(options != nullptr, "no options");
    TsdfGrid G;
    int rc;
    if ((rc = check_volume_grid("smvs_tsdf_sparse_volume_create", *options, 4096, G)))
        return rc;
    size_t n_bricks;
    TsdfBricks const B = brick_grid(G, &n_bricks);
    SMVS_REQUIRE(n_bricks <= MAX_BRICKS_GRID, "the brick grid has more than 2^28 bricks");
    int64_t max_bricks = options->max_bricks;
    if (max_bricks <= 0)
        max_bricks = DEFAULT_MAX_BRICKS;
    SMVS_REQUIRE(max_bricks <= MAX_MAX_BRICKS, "max_bricks must be at most 2^23");

    WorkspaceLease lease(device);
    if (lease.w == nullptr)
        return SMVS_ERR_HIP;
    smvs_tsdf_sparse_volume *vol = new (std::nothrow) smvs_tsdf_sparse_volume();
    if (vol == nullptr) {
        set_error("smvs_tsdf_sparse_volume_create: out of host memory");
        return SMVS_ERR_NOMEM;
    }
    vol->device = device;
    vol->options = *options;
    vol->G = G;
    vol->B = B;
    vol->n_bricks = n_bricks;
    vol->max_bricks = max_bricks;
    if ((rc = device_malloc(reinterpret_cast<void **>(&vol->seed), padded(n_bricks)))
        || (rc = device_malloc(reinterpret_cast<void **>(&vol->table), 4 * n_bricks))
        || (rc = empty_state(*lease.w, *vol))) {
        free_volume(vol);
        return rc;
    }
    *volume = vol;
    return SMVS_OK;
}

extern "C" int
smvs_tsdf_sparse_volume_mark(smvs_tsdf_sparse_volume *volume, const smvs_point_view *views,
    int n_views, int cut_surfaces, int cull)
{
    SMVS_REQUIRE(volume != nullptr, "no volume");
    int rc;
    if ((rc = check_views(views, n_views, cut_surfaces, false)))
        return rc;
    return run("smvs_tsdf_sparse_volume_mark", *volume, views, n_views, cut_surfaces != 0,
        cull != 0, true, false);
}

extern "C" int
smvs_tsdf_sparse_volume_integrate(smvs_tsdf_sparse_volume *volume, const smvs_point_view *views,
    int n_views, int cut_surfaces, int grow, int cull)
{
    SMVS_REQUIRE(volume != nullptr, "no volume");
    int rc;
    if ((rc = check_views(views, n_views, cut_surfaces, true)))
        return rc;
    SMVS_REQUIRE(volume->n_views + n_views <= VOLUME_MAX_VIEWS,
        "more than 2^24 views in one volume");
    return run("smvs_tsdf_sparse_volume_integrate", *volume, views, n_views, cut_surfaces != 0,
        cull != 0, grow != 0, true);
}

extern "C" int
smvs_tsdf_sparse_volume_extract(const smvs_tsdf_sparse_volume *volume, int min_weight,
    uint8_t *brick_state, float *tsdf, uint32_t *weight, smvs_points **handle,
    int64_t *n_vertices, int64_t *n_faces)
{
    SMVS_REQUIRE(handle != nullptr, "no handle pointer");
    *handle = nullptr;
    SMVS_REQUIRE(volume != nullptr, "no volume");
    TsdfGrid G = volume->G;
    G.min_weight = min_weight > 0 ? (uint32_t)min_weight : 1u;
    G.n_views = (int)volume->n_views;
    size_t const n_vox = (size_t)G.nx * G.ny * G.nz;
    SMVS_REQUIRE((tsdf == nullptr && weight == nullptr) || n_vox <= TSDF_MAX_VOXELS,
        "tsdf / weight are given only for grids of at most 2^27 voxels");
    size_t const n_bricks = volume->n_bricks, n_slots = volume->n_slots;

    WorkspaceLease lease(volume->device);
    if (lease.w == nullptr)
        return SMVS_ERR_HIP;
    Workspace &ws = *lease.w;
    Carver carve;
    size_t const tsdf_at = carve(4 * 256 * n_slots);
    size_t const state_at = carve(brick_state != nullptr ? n_bricks : 0),
        counts_at = carve(brick_state != nullptr ? 8 * ((n_bricks + 255) / 256) : 0);
    char *slab = nullptr;
    int rc;
    if ((rc = ws.ensure(0, carve.total > 0 ? carve.total : 256, &slab)) != SMVS_OK)
        return rc;
    if (brick_state != nullptr) {
        uint8_t *d_state = reinterpret_cast<uint8_t *>(slab + state_at);
        launch_dilate(ws.stream, volume->seed, volume->B, d_state,
            reinterpret_cast<unsigned long long *>(slab + counts_at));
        SMVS_HIP_CHECK(hipGetLastError());
        if ((rc = ws.download(brick_state, d_state, n_bricks)))
            return rc;
    }
    float *d_tsdf = reinterpret_cast<float *>(slab + tsdf_at);
    if (n_slots > 0)
        hipLaunchKernelGGL(tsdf_sparse_volume_field_kernel, dim3((unsigned)n_slots), dim3(256), 0,
            ws.stream, volume->S, volume->W, G.min_weight, d_tsdf);
    smvs_points *h = nullptr;
    if ((rc = extract_sparse_surface(ws, "smvs_tsdf_sparse_volume_extract", G, volume->B, n_slots,
            d_tsdf, volume->W, volume->colour, volume->table, volume->list, tsdf, weight, &h)))
        return rc;
    // (fill_points has drained the stream)
    return publish(h, handle, n_vertices, n_faces);
}

extern "C" int
smvs_tsdf_sparse_volume_info(const smvs_tsdf_sparse_volume *volume,
    smvs_tsdf_sparse_volume_options *options, smvs_tsdf_sparse_volume_stats *stats, int *device)
{
    SMVS_REQUIRE(volume != nullptr, "no volume");
    if (options != nullptr)
        *options = volume->options;
    if (stats != nullptr) {
        stats->bricks = (int64_t)volume->n_bricks;
        stats->seed_bricks = (int64_t)volume->n_seeds;
        stats->allocated_bricks = (int64_t)volume->n_slots;
        stats->pending_bricks = (int64_t)(volume->n_dilated - volume->n_slots);
        stats->late_bricks = (int64_t)volume->n_late;
        stats->state_bytes = (int64_t)volume->n_slots * VOLUME_STATE_BYTES_PER_BRICK;
        stats->n_views = volume->n_views;
    }
    if (device != nullptr)
        *device = volume->device;
    return SMVS_OK;
}

extern "C" int
smvs_tsdf_sparse_volume_download(const smvs_tsdf_sparse_volume *volume, uint8_t *brick_state,
    uint32_t *list, uint32_t *birth, float *S, uint32_t *W, uint32_t *rgbc)
{
    SMVS_REQUIRE(volume != nullptr, "no volume");
    WorkspaceLease lease(volume->device);
    if (lease.w == nullptr)
        return SMVS_ERR_HIP;
    Workspace &ws = *lease.w;
    size_t const n_bricks = volume->n_bricks, n_slots = volume->n_slots, n_state = 256 * n_slots;
    int rc;
    if (brick_state != nullptr) {
        Carver carve;
        size_t const state_at = carve(n_bricks), counts_at = carve(8 * ((n_bricks + 255) / 256));
        char *slab = nullptr;
        if ((rc = ws.ensure(0, carve.total, &slab)) != SMVS_OK)
            return rc;
        uint8_t *d_state = reinterpret_cast<uint8_t *>(slab + state_at);
        launch_dilate(ws.stream, volume->seed, volume->B, d_state,
            reinterpret_cast<unsigned long long *>(slab + counts_at));
        SMVS_HIP_CHECK(hipGetLastError());
        if ((rc = ws.download(brick_state, d_state, n_bricks)))
            return rc;
    }
    if ((list != nullptr && (rc = ws.download(list, volume->list, 4 * n_slots)))
        || (birth != nullptr && (rc = ws.download(birth, volume->birth, 4 * n_slots)))
        || (S != nullptr && (rc = ws.download(S, volume->S, 4 * n_state)))
        || (W != nullptr && (rc = ws.download(W, volume->W, 4 * n_state)))
        || (rgbc != nullptr && (rc = ws.download(rgbc, volume->colour, 16 * n_state))))
        return rc;
    return SMVS_OK;
}

extern "C" int
smvs_tsdf_sparse_volume_upload(smvs_tsdf_sparse_volume *volume, const uint8_t *brick_state,
    const uint32_t *list, const uint32_t *birth, int64_t n_slots, const float *S,
    const uint32_t *W, const uint32_t *rgbc, int64_t n_views)
{
    SMVS_REQUIRE(volume != nullptr, "no volume");
    SMVS_REQUIRE(brick_state != nullptr, "no state");
    SMVS_REQUIRE(n_views >= 0 && n_views <= VOLUME_MAX_VIEWS, "n_views must be 0 .. 2^24");
    SMVS_REQUIRE(n_slots >= 0 && n_slots <= volume->max_bricks, "n_slots must be 0 .. max_bricks");
    SMVS_REQUIRE(n_slots == 0 || (list != nullptr && birth != nullptr && S != nullptr
        && W != nullptr && rgbc != nullptr), "no state");
    smvs_tsdf_sparse_volume &vol = *volume;
    TsdfBricks const B = vol.B;
    size_t const n_bricks = vol.n_bricks;
    // the seeds, and their dilation with its count
    std::vector<uint8_t> seed(padded(n_bricks), 0), dilated(n_bricks, 0);
    size_t n_seeds = 0, n_dilated = 0;
    for (size_t brick = 0; brick < n_bricks; ++brick) {
        SMVS_REQUIRE(brick_state[brick] <= 2, "brick_state must be 0, 1 or 2");
        if (brick_state[brick] != 2)
            continue;
        seed[brick] = 2;
        ++n_seeds;
        int const bi = (int)(brick % B.bx), bj = (int)(brick / B.bx % B.by),
            bk = (int)(brick / B.bx / B.by);
        for (int dk = -1; dk <= 1; ++dk)
            for (int dj = -1; dj <= 1; ++dj)
                for (int di = -1; di <= 1; ++di) {
                    int const ni = bi + di, nj = bj + dj, nk = bk + dk;
                    if (ni < 0 || nj < 0 || nk < 0 || ni >= B.bx || nj >= B.by || nk >= B.bz)
                        continue;
                    uint8_t &d = dilated[((size_t)nk * B.by + nj) * B.bx + ni];
                    n_dilated += d == 0;
                    d = 1;
                }
    }
    SMVS_REQUIRE((int64_t)n_dilated <= vol.max_bricks,
        "the seeds' dilation has more than max_bricks bricks");
    size_t n_late = 0;
    for (int64_t slot = 0; slot < n_slots; ++slot) {
        SMVS_REQUIRE(list[slot] < n_bricks, "a list entry is outside the grid");
        SMVS_REQUIRE(slot == 0 || list[slot - 1] < list[slot], "the list must be strictly ascending");
        SMVS_REQUIRE(dilated[list[slot]] != 0, "a list entry is outside the seeds' dilation");
        SMVS_REQUIRE((int64_t)birth[slot] <= n_views, "a birth is above n_views");
        n_late += birth[slot] > 0;
    }

    WorkspaceLease lease(vol.device);
    if (lease.w == nullptr)
        return SMVS_ERR_HIP;
    Workspace &ws = *lease.w;
    int rc;
    Planes fresh;
    size_t const slots = (size_t)n_slots, n_state = 256 * slots;
    if (slots > 0) {
        if ((rc = alloc_planes(slots, fresh)))
            return rc;
        if ((rc = ws.upload(fresh.list, list, 4 * slots))
            || (rc = ws.upload(fresh.birth, birth, 4 * slots))
            || (rc = ws.upload(fresh.S, S, 4 * n_state)) || (rc = ws.upload(fresh.W, W, 4 * n_state))
            || (rc = ws.upload(fresh.colour, rgbc, 16 * n_state))) {
            (void)hipStreamSynchronize(ws.stream);
            free_planes(fresh);
            return rc;
        }
    }
    // (from here on a failure leaves undefined seeds and table: reset or upload again)
    hipError_t err = hipMemsetAsync(vol.table, 0xff, 4 * n_bricks, ws.stream);
    if (err == hipSuccess && slots > 0) {
        hipLaunchKernelGGL(tsdf_sparse_volume_scatter_kernel, dim3((unsigned)((slots + 255) / 256)),
            dim3(256), 0, ws.stream, fresh.list, slots, vol.table);
        err = hipGetLastError();
    }
    rc = err == hipSuccess ? ws.upload(vol.seed, seed.data(), padded(n_bricks)) : SMVS_ERR_HIP;
    if (rc == SMVS_OK && (err = hipStreamSynchronize(ws.stream)) != hipSuccess)
        rc = SMVS_ERR_HIP;
    if (rc != SMVS_OK) {
        if (err != hipSuccess)
            set_error("smvs_tsdf_sparse_volume_upload: %s", hipGetErrorString(err));
        (void)hipStreamSynchronize(ws.stream);
        free_planes(fresh);
        return rc;
    }
    adopt_planes(vol, fresh, slots);
    vol.n_seeds = n_seeds;
    vol.n_dilated = n_dilated;
    vol.n_late = n_late;
    vol.n_views = n_views;
    return SMVS_OK;
}

extern "C" int
smvs_tsdf_sparse_volume_reset(smvs_tsdf_sparse_volume *volume)
{
    SMVS_REQUIRE(volume != nullptr, "no volume");
    WorkspaceLease lease(volume->device);
    if (lease.w == nullptr)
        return SMVS_ERR_HIP;
    return empty_state(*lease.w, *volume);
}

extern "C" void
smvs_tsdf_sparse_volume_release(smvs_tsdf_sparse_volume *volume)
{
    if (volume != nullptr)
        free_volume(volume);
}
