// What every scene-export path shares behind its own passes (export_shared.h):
// the 64-bit exclusive scan that orders vertices and faces without atomics,
// smvsrecon's AABB vertex clip (app/smvsrecon.cc:306-319), the fill of the
// result handle and the handle's accessors.
#include "common.h"
#include "export_shared.h"
#include "mesh_shared.h"

#include <vector>

namespace smvs_hip {

// ------------------------------------------------------------ exclusive scan
// of n 64-bit values in place: 4096 per tile (256 threads x 16), a tile pass,
// one workgroup over the tile sums, a second tile pass; order fixed, no atomics

__device__ __forceinline__ unsigned long long
block_exclusive_scan(unsigned long long v, unsigned long long *total)
{
    __shared__ unsigned long long wsum[4];
    int const lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        unsigned long long const t = __shfl_up(inc, o, 64);
        if (lane >= o)
            inc += t;
    }
    if (lane == 63)
        wsum[wave] = inc;
    __syncthreads();
    unsigned long long pre = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        pre += k < wave ? wsum[k] : 0ull;
        tot += wsum[k];
    }
    __syncthreads();
    *total = tot;
    return pre + inc - v;
}

__global__ void __launch_bounds__(256)
scan_tile_sums_kernel(const unsigned long long *__restrict__ a, size_t n,
    unsigned long long *__restrict__ tiles)
{
    size_t const at = (size_t)blockIdx.x * SCAN_TILE + (size_t)threadIdx.x * SCAN_ITEMS;
    unsigned long long s = 0;
    for (int k = 0; k < SCAN_ITEMS; ++k)
        if (at + k < n)
            s += a[at + k];
    unsigned long long tot;
    (void)block_exclusive_scan(s, &tot);
    if (threadIdx.x == 0)
        tiles[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(256)
scan_tiles_kernel(unsigned long long *tiles, size_t n_tiles)
{
    unsigned long long carry = 0;
    for (size_t at = 0; at < n_tiles; at += 256) {
        size_t const i = at + threadIdx.x;
        unsigned long long const v = i < n_tiles ? tiles[i] : 0ull;
        unsigned long long tot;
        unsigned long long const ex = block_exclusive_scan(v, &tot);
        if (i < n_tiles)
            tiles[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0)
        tiles[n_tiles] = carry;
}

__global__ void __launch_bounds__(256)
scan_apply_kernel(unsigned long long *a, size_t n,
    const unsigned long long *__restrict__ tiles)
{
    size_t const at = (size_t)blockIdx.x * SCAN_TILE + (size_t)threadIdx.x * SCAN_ITEMS;
    unsigned long long vals[SCAN_ITEMS];
    unsigned long long s = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        vals[k] = at + k < n ? a[at + k] : 0ull;
        s += vals[k];
    }
    unsigned long long tot;
    unsigned long long run = block_exclusive_scan(s, &tot) + tiles[blockIdx.x];
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        if (at + k < n)
            a[at + k] = run;
        run += vals[k];
    }
}

int
exclusive_scan(hipStream_t stream, unsigned long long *a, size_t n,
    unsigned long long *tiles)
{
    size_t const n_tiles = (n + SCAN_TILE - 1) / SCAN_TILE;
    hipLaunchKernelGGL(scan_tile_sums_kernel, dim3((unsigned)n_tiles), dim3(256), 0,
        stream, a, n, tiles);
    hipLaunchKernelGGL(scan_tiles_kernel, dim3(1), dim3(256), 0, stream, tiles, n_tiles);
    hipLaunchKernelGGL(scan_apply_kernel, dim3((unsigned)n_tiles), dim3(256), 0,
        stream, a, n, tiles);
    SMVS_HIP_CHECK(hipGetLastError());
    return SMVS_OK;
}

// ------------------------------------------------------------------ AABB clip
__global__ void __launch_bounds__(256)
aabb_keep_kernel(const float *__restrict__ xyz, size_t n, float3 lo, float3 hi,
    unsigned long long *__restrict__ keep)
{
    size_t const i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    keep[i] = outside_aabb(xyz + 3 * i, lo, hi) ? 0ull : 1ull;
}

__global__ void __launch_bounds__(256)
aabb_compact_kernel(size_t n, float3 lo, float3 hi,
    const unsigned long long *__restrict__ at, VertexAttrs src, VertexAttrs dst)
{
    size_t const i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    if (outside_aabb(src.xyz + 3 * i, lo, hi))
        return;
    size_t const j = at[i];
    SMVS_COPY_VERTEX(src, i, dst, j);
}

int
launch_aabb_clip(hipStream_t stream, size_t n, float3 lo, float3 hi, VertexAttrs src,
    VertexAttrs dst, unsigned long long *scan, unsigned long long *tiles)
{
    unsigned const blocks = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(aabb_keep_kernel, dim3(blocks), dim3(256), 0, stream, src.xyz, n, lo,
        hi, scan);
    SMVS_HIP_CHECK(hipGetLastError());
    int const rc = exclusive_scan(stream, scan, n, tiles);
    if (rc != SMVS_OK)
        return rc;
    hipLaunchKernelGGL(aabb_compact_kernel, dim3(blocks), dim3(256), 0, stream, n, lo, hi,
        scan, src, dst);
    SMVS_HIP_CHECK(hipGetLastError());
    return SMVS_OK;
}

// ---------------------------------------------------------------- result fill
int
fill_points(Workspace &ws, bool mesh, bool sparse, size_t n_vert, size_t n_face,
    VertexAttrs const &v, const uint32_t *faces, const long long *cells, smvs_points **handle)
{
    smvs_points *h = new smvs_points;
    h->mesh = mesh;
    h->sparse = sparse;
    h->n_points = (int64_t)n_vert;
    h->n_faces = faces != nullptr ? (int64_t)n_face : 0;
    size_t const nv = n_vert, nf = (size_t)h->n_faces;
    h->xyz.resize(3 * nv);
    h->nrm.resize(3 * nv);
    h->rgb.resize(3 * nv);
    h->conf.resize(nv);
    h->val.resize(v.val != nullptr ? nv : 0);
    h->cells.resize(cells != nullptr ? nv : 0);
    h->faces.resize(3 * nf);
    int rc;
    if ((rc = ws.download(h->xyz.data(), v.xyz, 12 * nv))
        || (rc = ws.download(h->nrm.data(), v.nrm, 12 * nv))
        || (rc = ws.download(h->rgb.data(), v.rgb, 3 * nv))
        || (rc = ws.download(h->conf.data(), v.conf, 4 * nv))
        || (rc = ws.download(h->val.data(), v.val, 4 * h->val.size()))
        || (rc = ws.download(h->cells.data(), cells, 8 * h->cells.size()))
        || (rc = ws.download(h->faces.data(), faces, 12 * nf))) {
        delete h;
        return rc;
    }
    *handle = h;
    return SMVS_OK;
}

} // namespace smvs_hip

using namespace smvs_hip;

extern "C" int
smvs_points_info(const smvs_points *handle, int64_t *n_points, int64_t *n_faces)
{
    SMVS_REQUIRE(handle != nullptr, "no handle");
    if (n_points != nullptr)
        *n_points = handle->n_points;
    if (n_faces != nullptr)
        *n_faces = handle->n_faces;
    return SMVS_OK;
}

extern "C" int
smvs_points_download(const smvs_points *handle, float *xyz, float *normals,
    uint8_t *rgb, float *confidence, float *value, uint32_t *faces)
{
    SMVS_REQUIRE(handle != nullptr, "no handle");
    SMVS_REQUIRE(!(handle->mesh && value != nullptr),
        "a triangle mesh has no values");
    auto copy = [](void *dst, auto const &src) {
        if (dst != nullptr && !src.empty())
            memcpy(dst, src.data(), src.size() * sizeof(src[0]));
    };
    copy(xyz, handle->xyz);
    copy(normals, handle->nrm);
    copy(rgb, handle->rgb);
    copy(confidence, handle->conf);
    copy(value, handle->val);
    copy(faces, handle->faces);
    return SMVS_OK;
}

extern "C" int
smvs_points_release(smvs_points *handle)
{
    delete handle;
    return SMVS_OK;
}
