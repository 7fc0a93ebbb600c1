// Speckle removal on a depth map on gfx950 (not in the reference;
// include/smvs_hip.h, "speckle removal", has the definition): connected
// components of the valid pixels under the ratio link, every component smaller
// than speckle_size set to 0.
//
// A union-find over pixel indices in four launches, none of which waits for
// another workgroup:
//   tile    one workgroup per 32 x 32 tile: union-find of the tile in LDS
//           (atomicMin on roots), labels written as global pixel indices; the
//           component counts zeroed;
//   border  one thread per linked pair across a tile edge: the same union on
//           the global labels (skipped for a map of one tile);
//   count   every valid pixel flattened to its root, one integer atomicAdd per
//           (wave, root of the wave's first valid lane) and per other pixel;
//   apply   the threshold; `size` written over the labels.
// Invariant of every union: a parent's index is never larger than the pixel's
// own and a label only ever decreases (atomicMin), so every find loop ends at a
// pixel that is its own parent, whatever it read on the way.  The partition is
// a fact of the input and the counts are integer sums: the result is defined
// to the bit.
#include "sgm_internal.h"
#include "union_find.h"

namespace smvs_hip {

constexpr int SP_TILE = 32;                       // tile edge in pixels
constexpr int SP_TILE_PIX = SP_TILE * SP_TILE;
constexpr int SP_THREADS = 256;

// two 4-neighbours are linked: both valid (a NaN is not) and the ratio test of
// the consensus, one IEEE division
__device__ __forceinline__ bool
speckle_linked(float a, float b, float ratio)
{
#pragma clang fp contract(off)
    return a > 0.0f && b > 0.0f && fminf(a, b) / fmaxf(a, b) >= ratio;
}

// (uf_find and uf_union: union_find.h; workgroup scope for the labels of a tile
// in LDS, agent scope for the global labels)

// label[p], p = y * w + x: the root of p inside its tile as a global pixel
// index (a pixel that is not valid is its own root); count[p] = 0.
__global__ void __launch_bounds__(SP_THREADS)
speckle_tile_kernel(const float *depth, int w, int h, float ratio, uint32_t *label,
    uint32_t *count)
{
    __shared__ float tile[SP_TILE_PIX];
    __shared__ uint32_t lab[SP_TILE_PIX];
    int const tiles_x = (w + SP_TILE - 1) / SP_TILE;
    int const x0 = (int)(blockIdx.x % (unsigned)tiles_x) * SP_TILE;
    int const y0 = (int)(blockIdx.x / (unsigned)tiles_x) * SP_TILE;
    int const tid = (int)threadIdx.x;
    for (int i = tid; i < SP_TILE_PIX; i += SP_THREADS) {
        int const gx = x0 + (i & (SP_TILE - 1)), gy = y0 + i / SP_TILE;
        tile[i] = gx < w && gy < h ? depth[(size_t)gy * w + gx] : 0.0f;
        lab[i] = (uint32_t)i;
    }
    __syncthreads();
    for (int i = tid; i < SP_TILE_PIX; i += SP_THREADS) {
        float const d = tile[i];
        if ((i & (SP_TILE - 1)) != 0 && speckle_linked(d, tile[i - 1], ratio))
            uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, (uint32_t)i, (uint32_t)(i - 1));
        if (i >= SP_TILE && speckle_linked(d, tile[i - SP_TILE], ratio))
            uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, (uint32_t)i, (uint32_t)(i - SP_TILE));
    }
    __syncthreads();
    for (int i = tid; i < SP_TILE_PIX; i += SP_THREADS) {
        int const gx = x0 + (i & (SP_TILE - 1)), gy = y0 + i / SP_TILE;
        if (gx >= w || gy >= h)
            continue;
        // (the raster order of a tile is the raster order of the map: a root
        // below i in the tile is a pixel below p in the map)
        uint32_t const r = uf_find<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, (uint32_t)i);
        size_t const p = (size_t)gy * w + gx;
        label[p] = (uint32_t)(y0 + (int)(r / SP_TILE)) * (uint32_t)w
            + (uint32_t)(x0 + (int)(r & (SP_TILE - 1)));
        count[p] = 0u;
    }
}

// The pairs across tile edges: (tiles_x - 1) * h pairs (x, x - 1) with x a
// multiple of the tile edge, then (tiles_y - 1) * w pairs (y, y - 1).
__global__ void __launch_bounds__(SP_THREADS)
speckle_border_kernel(const float *depth, int w, int h, float ratio, uint32_t *label)
{
    size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t const n_vert = (size_t)((w - 1) / SP_TILE) * (size_t)h;
    size_t const n_horz = (size_t)((h - 1) / SP_TILE) * (size_t)w;
    size_t p, q;
    if (j < n_vert) {
        size_t const x = (j / (size_t)h + 1) * SP_TILE, y = j % (size_t)h;
        p = y * (size_t)w + x;
        q = p - 1;
    } else {
        j -= n_vert;
        if (j >= n_horz)
            return;
        size_t const y = (j / (size_t)w + 1) * SP_TILE, x = j % (size_t)w;
        p = y * (size_t)w + x;
        q = p - (size_t)w;
    }
    if (speckle_linked(depth[p], depth[q], ratio))
        uf_union<__HIP_MEMORY_SCOPE_AGENT>(label, (uint32_t)p, (uint32_t)q);
}

// Every valid pixel to its root (no union runs any more: the roots are final)
// and the roots' counts.  The lanes of a wave that share the root of its first
// valid lane add once -- a large component is most of every wave it touches --
// the others one each.  (217 of the 307 us of the four launches at 960 x 540,
// where one component has 264 k pixels.  Letting one lane per wave walk for the
// lanes with its label did not change that, so it is not the number of loads;
// the walk itself, from a tile root through the chain of tile roots the border
// kernel built, is what is left to look at.)
__global__ void __launch_bounds__(SP_THREADS)
speckle_count_kernel(const float *depth, size_t npix, uint32_t *label, uint32_t *count)
{
    size_t const p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool const valid = p < npix && depth[p] > 0.0f;
    uint32_t r = 0u;
    if (valid) {
        r = uf_find<__HIP_MEMORY_SCOPE_AGENT>(label, (uint32_t)p);
        __hip_atomic_store(label + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    unsigned long long const any = __ballot(valid);
    if (any == 0ull)
        return;
    int const first = __ffsll((long long)any) - 1;
    uint32_t const lead = (uint32_t)__shfl((int)r, first);
    bool const with_lead = valid && r == lead;
    unsigned long long const group = __ballot(with_lead);
    int const lane = (int)(threadIdx.x & 63u);
    if (with_lead) {
        if (lane == first)
            atomicAdd(count + lead, (uint32_t)__popcll(group));
    } else if (valid) {
        atomicAdd(count + r, 1u);
    }
}

// out = 0 where 0 < size < speckle_size, the input's bits elsewhere; size
// (may be null) = the component's pixel count, 0 for a pixel that is not valid.
// `out` may be `depth`, `size` may be `label` (a thread reads and writes its
// own pixel).
__global__ void __launch_bounds__(SP_THREADS)
speckle_apply_kernel(const float *depth, size_t npix, const uint32_t *label,
    const uint32_t *count, uint32_t speckle_size, float *out, uint32_t *size)
{
    size_t const p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix)
        return;
    float const d = depth[p];
    uint32_t const s = d > 0.0f ? count[label[p]] : 0u;
    out[p] = s != 0u && s < speckle_size ? 0.0f : d;
    if (size != nullptr)
        size[p] = s;
}

// (declared in sgm_internal.h)
int
check_sgm_speckle(int speckle_size, float speckle_ratio)
{
    SMVS_REQUIRE(speckle_size >= 0, "speckle_size must not be negative");
    // (a NaN fails both comparisons)
    SMVS_REQUIRE(speckle_ratio >= 0.0f && speckle_ratio <= 1.0f,
        "speckle_ratio must be in [0, 1]");
    return SMVS_OK;
}

// (declared in sgm_internal.h)
int
sgm_speckle_ensure(Workspace &ws, size_t npix, uint32_t **d_words)
{
    return ws.ensure(WS_SPECKLE, 2 * npix, d_words);
}

// (declared in sgm_internal.h)
int
sgm_launch_speckle(Workspace &ws, SgmProfile *prof, const float *d_depth, int w, int h,
    int speckle_size, float speckle_ratio, uint32_t *d_words, float *d_out, bool want_size)
{
    hipStream_t const stream = ws.stream;
    size_t const npix = (size_t)w * h;
    uint32_t *const label = d_words, *const count = d_words + npix;
    unsigned const tiles = (unsigned)(((w + SP_TILE - 1) / SP_TILE) * ((h + SP_TILE - 1) / SP_TILE));
    size_t const pairs = (size_t)((w - 1) / SP_TILE) * (size_t)h
        + (size_t)((h - 1) / SP_TILE) * (size_t)w;
    unsigned const blocks = (unsigned)((npix + SP_THREADS - 1) / SP_THREADS);
    {
        SgmKernelTimer timer(prof, stream, SMVS_SGM_K_MERGE);
        hipLaunchKernelGGL(speckle_tile_kernel, dim3(tiles), dim3(SP_THREADS), 0, stream, d_depth,
            w, h, speckle_ratio, label, count);
    }
    if (pairs != 0) {
        SgmKernelTimer timer(prof, stream, SMVS_SGM_K_MERGE);
        hipLaunchKernelGGL(speckle_border_kernel,
            dim3((unsigned)((pairs + SP_THREADS - 1) / SP_THREADS)), dim3(SP_THREADS), 0, stream,
            d_depth, w, h, speckle_ratio, label);
    }
    {
        SgmKernelTimer timer(prof, stream, SMVS_SGM_K_MERGE);
        hipLaunchKernelGGL(speckle_count_kernel, dim3(blocks), dim3(SP_THREADS), 0, stream,
            d_depth, npix, label, count);
    }
    {
        SgmKernelTimer timer(prof, stream, SMVS_SGM_K_MERGE);
        hipLaunchKernelGGL(speckle_apply_kernel, dim3(blocks), dim3(SP_THREADS), 0, stream,
            d_depth, npix, label, count, (uint32_t)speckle_size, d_out,
            want_size ? label : nullptr);
    }
    SMVS_HIP_CHECK(hipGetLastError());
    return SMVS_OK;
}

} // namespace smvs_hip

using namespace smvs_hip;

// the kernels alone, on a map of the caller
extern "C" int
smvs_sgm_filter_speckles(int device, const float *depth, int w, int h, int speckle_size,
    float speckle_ratio, float *out, uint32_t *size)
{
    if (int const rc = check_sgm_speckle(speckle_size, speckle_ratio); rc != SMVS_OK)
        return rc;
    SMVS_REQUIRE(depth && out, "null argument");
    SMVS_REQUIRE(w >= 1 && h >= 1 && (size_t)w * h < ((size_t)1 << 31), "bad map size");
    int rc;
    WorkspaceLease lease(device);
    if (lease.w == nullptr)
        return SMVS_ERR_HIP;
    Workspace &ws = *lease.w;
    SgmProfile prof;
    size_t const npix = (size_t)w * h;
    float *d_depth = nullptr;
    uint32_t *d_words = nullptr;
    if ((rc = ws.ensure(WS_FWD0, npix, &d_depth)) || (rc = sgm_speckle_ensure(ws, npix, &d_words))
        || (rc = ws.upload(d_depth, depth, sizeof(float) * npix))
        || (rc = sgm_launch_speckle(ws, &prof, d_depth, w, h, speckle_size, speckle_ratio,
                d_words, d_depth, size != nullptr))
        || (rc = ws.download(out, d_depth, sizeof(float) * npix)))
        return rc;
    if (size != nullptr && (rc = ws.download(size, d_words, sizeof(uint32_t) * npix)))
        return rc;
    SMVS_HIP_CHECK(hipStreamSynchronize(ws.stream));
    return SMVS_OK;
}
