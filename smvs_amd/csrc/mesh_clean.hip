// Mesh clean on gfx950 (not in the reference; include/smvs_hip.h, "Cleaning a
// triangle mesh", has the definition): a cut on the
// vertex confidences, connected components over the surviving faces, and the
// order-preserving compaction of what remains.
//
// All launches are enqueued by launch_mesh_clean, none waits for another
// workgroup, nothing comes back to the host in between:
//   init      the counters, the select's state, t = threshold (or -inf)
//   select    percentile only, four times: a 256-bin histogram per block in LDS
//             of the key byte of the vertices that share the prefix found so
//             far, added to the global histogram; one workgroup scans the
//             bins, picks the one that holds the k-th key and descends one byte
//   vertices  cut per vertex, label[v] = v
//   faces     survive per face, referenced per corner (every writer stores 1)
//   union     one lane per surviving face unites (a, b) and (b, c)
//             (union_find.h, agent scope)
//   count     every uncut vertex flattened to its root, wave-aggregated adds
//   apply     small / unreferenced -> the keep flags, the statistics
//   scan, compact, face keep, scan, face compact (export_common.hip's scan,
//   SMVS_COPY_VERTEX of the AABB clip)
// The partition is a fact of the input and the counts are integer sums: the
// result is defined to the bit.
#include "export_shared.h"
#include "union_find.h"

#include <cmath>

namespace smvs_hip {

constexpr int MC_THREADS = 256;
constexpr unsigned MC_SELECT_BLOCKS = 2048;   // grid of the histogram passes at most
// words of MeshCleanWork::select: the key prefix found so far, k (64 bits, the
// rank wanted among the keys with that prefix), the global histogram
constexpr int MC_SEL_PREFIX = 0, MC_SEL_K = 2, MC_SEL_HIST = 4, MC_SEL_WORDS = 4 + 256;

// the order-preserving key of a float's bits (surface_planes.hip's) and back
__device__ __forceinline__ uint32_t
float_key(uint32_t u)
{
    return u ^ ((u >> 31) != 0u ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ uint32_t
key_float(uint32_t key)
{
    return (key >> 31) != 0u ? key ^ 0x80000000u : ~key;
}

__global__ void __launch_bounds__(MC_THREADS)
clean_init_kernel(MeshCleanCounts *counts, uint32_t *select, unsigned long long k, float t)
{
    select[MC_SEL_HIST + threadIdx.x] = 0u;
    if (threadIdx.x != 0)
        return;
    select[MC_SEL_PREFIX] = 0u;
    select[MC_SEL_K] = (uint32_t)k;
    select[MC_SEL_K + 1] = (uint32_t)(k >> 32);
    MeshCleanCounts c = {};
    c.cut_value = t;
    *counts = c;
}

// pass 0 .. 3 looks at key byte 3 - pass of the keys whose higher bytes equal
// the prefix's
__global__ void __launch_bounds__(MC_THREADS)
clean_select_hist_kernel(const float *__restrict__ conf, size_t n, uint32_t *select, int pass)
{
    __shared__ uint32_t hist[256];
    hist[threadIdx.x] = 0u;
    __syncthreads();
    int const shift = 24 - 8 * pass;
    unsigned long long const prefix = (unsigned long long)select[MC_SEL_PREFIX] >> (shift + 8);
    size_t const stride = (size_t)gridDim.x * MC_THREADS;
    for (size_t i = (size_t)blockIdx.x * MC_THREADS + threadIdx.x; i < n; i += stride) {
        uint32_t const key = float_key(__float_as_uint(conf[i]));
        if (((unsigned long long)key >> (shift + 8)) == prefix)
            atomicAdd(&hist[(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    uint32_t const mine = hist[threadIdx.x];
    if (mine != 0u)
        atomicAdd(select + MC_SEL_HIST + threadIdx.x, mine);
}

// one workgroup, one bin per thread: an inclusive scan of the histogram in LDS;
// the thread whose bin holds rank k makes the prefix one byte longer and k
// relative to its bin; the histogram is zero again; after the last byte the
// prefix is the key of t.  (n < 2^31: the sums fit 32 bits.  Every thread
// reads k and the prefix before the scan's barriers, the one writer writes
// behind them.)
__global__ void __launch_bounds__(MC_THREADS)
clean_select_pick_kernel(uint32_t *select, MeshCleanCounts *counts, int pass)
{
    __shared__ uint32_t upto[256];
    uint32_t const bin = threadIdx.x;
    uint32_t const mine = select[MC_SEL_HIST + bin];
    unsigned long long const k = (unsigned long long)select[MC_SEL_K]
        | ((unsigned long long)select[MC_SEL_K + 1] << 32);
    uint32_t const before = select[MC_SEL_PREFIX];
    select[MC_SEL_HIST + bin] = 0u;
    upto[bin] = mine;
    __syncthreads();
    for (uint32_t o = 1; o < 256u; o <<= 1) {
        uint32_t const left = bin >= o ? upto[bin - o] : 0u;
        __syncthreads();
        upto[bin] += left;
        __syncthreads();
    }
    uint32_t const through = upto[bin], below = through - mine;
    // (rank k lies in exactly one bin; the last bin also takes a k beyond the
    // total, which no caller passes)
    if (!((k >= below && k < through) || (bin == 255u && k >= through)))
        return;
    unsigned long long const rest = k - below;
    uint32_t const prefix = before | (bin << (24 - 8 * pass));
    select[MC_SEL_PREFIX] = prefix;
    select[MC_SEL_K] = (uint32_t)rest;
    select[MC_SEL_K + 1] = (uint32_t)(rest >> 32);
    if (pass == 3)
        counts->cut_value = __uint_as_float(key_float(prefix));
}

__device__ __forceinline__ void
wave_count(bool flag, unsigned long long *counter)
{
    unsigned long long const set = __ballot(flag);
    if (set != 0ull && (threadIdx.x & 63u) == (unsigned)(__ffsll((long long)set) - 1))
        atomicAdd(counter, (unsigned long long)__popcll(set));
}

__global__ void __launch_bounds__(MC_THREADS)
clean_vertex_flags_kernel(const float *__restrict__ conf, size_t n, MeshCleanCounts *counts,
    uint32_t *__restrict__ label, uint32_t *__restrict__ count, uint8_t *__restrict__ cut,
    uint8_t *__restrict__ referenced)
{
    size_t const i = (size_t)blockIdx.x * MC_THREADS + threadIdx.x;
    float const t = counts->cut_value;
    bool c = false;
    if (i < n) {
        c = conf[i] < t;   // (false for a NaN on either side)
        cut[i] = c ? 1 : 0;
        referenced[i] = 0;
        label[i] = (uint32_t)i;
        count[i] = 0u;
    }
    wave_count(c, &counts->n_cut);
}

__global__ void __launch_bounds__(MC_THREADS)
clean_face_flags_kernel(const uint32_t *__restrict__ faces, size_t m,
    const uint8_t *__restrict__ cut, uint8_t *referenced, uint8_t *__restrict__ survive)
{
    size_t const f = (size_t)blockIdx.x * MC_THREADS + threadIdx.x;
    if (f >= m)
        return;
    uint32_t const a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    bool const s = a != b && b != c && a != c && cut[a] == 0 && cut[b] == 0 && cut[c] == 0;
    survive[f] = s ? 1 : 0;
    if (s) {
        referenced[a] = 1;
        referenced[b] = 1;
        referenced[c] = 1;
    }
}

__global__ void __launch_bounds__(MC_THREADS)
clean_union_kernel(const uint32_t *__restrict__ faces, size_t m,
    const uint8_t *__restrict__ survive, uint32_t *label)
{
    size_t const f = (size_t)blockIdx.x * MC_THREADS + threadIdx.x;
    if (f >= m || survive[f] == 0)
        return;
    uint32_t const a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    uf_union<__HIP_MEMORY_SCOPE_AGENT>(label, a, b);
    uf_union<__HIP_MEMORY_SCOPE_AGENT>(label, b, c);
}

// Every uncut vertex to its root (no union runs any more: the roots are final)
// and the roots' counts, added as sgm_speckle.hip's count kernel adds them: the
// lanes of a wave that share the root of its first uncut lane add once.
__global__ void __launch_bounds__(MC_THREADS)
clean_count_kernel(size_t n, const uint8_t *__restrict__ cut, uint32_t *label, uint32_t *count)
{
    size_t const i = (size_t)blockIdx.x * MC_THREADS + threadIdx.x;
    bool const valid = i < n && cut[i] == 0;
    uint32_t r = 0u;
    if (valid) {
        r = uf_find<__HIP_MEMORY_SCOPE_AGENT>(label, (uint32_t)i);
        // (r is at or below every label this vertex ever had)
        (void)__hip_atomic_fetch_min(label + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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

// keep[i] (the scan's input) and removed[i] = !keep; label becomes the
// definition's `component`; size (may be null) its `component_size`.  `removed`
// may be `cut`: a thread reads and writes its own vertex.
__global__ void __launch_bounds__(MC_THREADS)
clean_apply_kernel(size_t n, const uint8_t *cut, const uint8_t *__restrict__ referenced,
    uint32_t *label, const uint32_t *__restrict__ count, uint32_t component_size,
    int keep_unreferenced, MeshCleanCounts *counts, uint32_t *__restrict__ size,
    uint8_t *removed, unsigned long long *__restrict__ keep)
{
    size_t const i = (size_t)blockIdx.x * MC_THREADS + threadIdx.x;
    bool const valid = i < n;
    bool const uncut = valid && cut[i] == 0;
    // (the count kernel left label[i] at the root: read by this thread alone
    // here, while other threads read count[] only)
    uint32_t const r = uncut ? label[i] : 0xFFFFFFFFu;
    uint32_t const s = uncut ? count[r] : 0u;
    bool const small = uncut && component_size > 1u && s < component_size;
    bool const unref = uncut && referenced[i] == 0;
    bool const kept = uncut && !small && (keep_unreferenced != 0 || !unref);
    bool const root = uncut && r == (uint32_t)i;
    if (valid) {
        keep[i] = kept ? 1ull : 0ull;
        removed[i] = kept ? 0 : 1;
        if (!uncut)
            label[i] = 0xFFFFFFFFu;
        if (size != nullptr)
            size[i] = s;
    }
    wave_count(root, &counts->n_components);
    wave_count(root && small, &counts->n_small_components);
    wave_count(small, &counts->n_small_vertices);
    wave_count(unref, &counts->n_unreferenced);
    // the wave's largest root size, one atomic per wave that holds a root
    uint32_t big = root ? s : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        uint32_t const other = (uint32_t)__shfl_xor((int)big, o, 64);
        big = other > big ? other : big;
    }
    if ((threadIdx.x & 63u) == 0u && big != 0u)
        atomicMax(&counts->largest_component, (unsigned long long)big);
}

// at: the scanned keep flags in, `new_id` (int64, -1 for a removed vertex) out
__global__ void __launch_bounds__(MC_THREADS)
clean_compact_kernel(size_t n, const uint8_t *__restrict__ removed, unsigned long long *at,
    VertexAttrs src, const long long *__restrict__ src_cells, VertexAttrs dst,
    long long *__restrict__ dst_cells)
{
    size_t const i = (size_t)blockIdx.x * MC_THREADS + threadIdx.x;
    if (i >= n)
        return;
    if (removed[i] != 0) {
        at[i] = ~0ull;
        return;
    }
    size_t const j = (size_t)at[i];
    SMVS_COPY_VERTEX(src, i, dst, j);
    if (src_cells != nullptr)
        dst_cells[j] = src_cells[i];
}

// second pass over the faces: a surviving face whose corners all remain
__global__ void __launch_bounds__(MC_THREADS)
clean_face_keep_kernel(const uint32_t *__restrict__ faces, size_t m, uint8_t *__restrict__ survive,
    const unsigned long long *__restrict__ new_id, unsigned long long *__restrict__ keep)
{
    size_t const f = (size_t)blockIdx.x * MC_THREADS + threadIdx.x;
    if (f >= m)
        return;
    bool k = survive[f] != 0;
    if (k) {
        for (int r = 0; r < 3; ++r)
            k = k && new_id[faces[3 * f + r]] != ~0ull;
    }
    survive[f] = k ? 1 : 0;
    keep[f] = k ? 1ull : 0ull;
}

__global__ void __launch_bounds__(MC_THREADS)
clean_face_compact_kernel(const uint32_t *__restrict__ faces, size_t m,
    const uint8_t *__restrict__ kept, const unsigned long long *__restrict__ at,
    const unsigned long long *__restrict__ new_id, uint32_t *__restrict__ dst)
{
    size_t const f = (size_t)blockIdx.x * MC_THREADS + threadIdx.x;
    if (f >= m || kept[f] == 0)
        return;
    size_t const j = (size_t)at[f];
    for (int r = 0; r < 3; ++r)
        dst[3 * j + r] = (uint32_t)new_id[faces[3 * f + r]];
}

// the two totals beside the counters (null: nothing was scanned, 0)
__global__ void
clean_totals_kernel(MeshCleanCounts *counts, const unsigned long long *n_vertices,
    const unsigned long long *n_faces)
{
    counts->n_vertices = n_vertices != nullptr ? *n_vertices : 0ull;
    counts->n_faces = n_faces != nullptr ? *n_faces : 0ull;
}

MeshCleanPieces
carve_mesh_clean(Carver &carve, size_t n, size_t m, bool want_size)
{
    MeshCleanPieces at = {};
    at.want_size = want_size;
    at.counts = carve(sizeof(MeshCleanCounts));
    at.select = carve(4 * MC_SEL_WORDS);
    at.label = carve(4 * n);
    at.count = carve(4 * n);
    at.size = want_size ? carve(4 * n) : 0;
    at.cut = carve(n);
    at.referenced = carve(n);
    at.survive = carve(m);
    at.vscan = carve(8 * n);
    at.vtiles = carve(8 * ((n + SCAN_TILE - 1) / SCAN_TILE + 1));
    at.fscan = carve(8 * m);
    at.ftiles = carve(8 * ((m + SCAN_TILE - 1) / SCAN_TILE + 1));
    return at;
}

MeshCleanWork
mesh_clean_work(char *slab, MeshCleanPieces const &at)
{
    MeshCleanWork w;
    w.counts = reinterpret_cast<MeshCleanCounts *>(slab + at.counts);
    w.select = reinterpret_cast<uint32_t *>(slab + at.select);
    w.label = reinterpret_cast<uint32_t *>(slab + at.label);
    w.count = reinterpret_cast<uint32_t *>(slab + at.count);
    w.size = at.want_size ? reinterpret_cast<uint32_t *>(slab + at.size) : nullptr;
    w.cut = reinterpret_cast<uint8_t *>(slab + at.cut);
    w.referenced = reinterpret_cast<uint8_t *>(slab + at.referenced);
    w.survive = reinterpret_cast<uint8_t *>(slab + at.survive);
    w.vscan = reinterpret_cast<unsigned long long *>(slab + at.vscan);
    w.vtiles = reinterpret_cast<unsigned long long *>(slab + at.vtiles);
    w.fscan = reinterpret_cast<unsigned long long *>(slab + at.fscan);
    w.ftiles = reinterpret_cast<unsigned long long *>(slab + at.ftiles);
    return w;
}

int
launch_mesh_clean(hipStream_t stream, size_t n, size_t m, VertexAttrs src,
    const long long *src_cells, const uint32_t *src_faces, smvs_mesh_clean_options const &opt,
    MeshCleanWork const &w, VertexAttrs dst, long long *dst_cells, uint32_t *dst_faces)
{
    bool const select = opt.percentile > 0.0f && n > 0;
    float t = -INFINITY;   // no cut
    if (opt.percentile == 0.0f && opt.threshold > 0.0f)
        t = opt.threshold;
    unsigned long long const k = select
        ? (unsigned long long)(long long)((double)opt.percentile * (double)(n - 1) / 100.0) : 0ull;
    hipLaunchKernelGGL(clean_init_kernel, dim3(1), dim3(MC_THREADS), 0, stream, w.counts,
        w.select, k, t);
    unsigned const vblocks = (unsigned)((n + MC_THREADS - 1) / MC_THREADS);
    unsigned const fblocks = (unsigned)((m + MC_THREADS - 1) / MC_THREADS);
    if (select) {
        unsigned const blocks = vblocks < MC_SELECT_BLOCKS ? vblocks : MC_SELECT_BLOCKS;
        for (int pass = 0; pass < 4; ++pass) {
            hipLaunchKernelGGL(clean_select_hist_kernel, dim3(blocks), dim3(MC_THREADS), 0,
                stream, src.conf, n, w.select, pass);
            hipLaunchKernelGGL(clean_select_pick_kernel, dim3(1), dim3(MC_THREADS), 0, stream,
                w.select, w.counts, pass);
        }
    }
    if (n > 0) {
        hipLaunchKernelGGL(clean_vertex_flags_kernel, dim3(vblocks), dim3(MC_THREADS), 0, stream,
            src.conf, n, w.counts, w.label, w.count, w.cut, w.referenced);
        if (m > 0) {
            hipLaunchKernelGGL(clean_face_flags_kernel, dim3(fblocks), dim3(MC_THREADS), 0,
                stream, src_faces, m, w.cut, w.referenced, w.survive);
            hipLaunchKernelGGL(clean_union_kernel, dim3(fblocks), dim3(MC_THREADS), 0, stream,
                src_faces, m, w.survive, w.label);
        }
        hipLaunchKernelGGL(clean_count_kernel, dim3(vblocks), dim3(MC_THREADS), 0, stream, n,
            w.cut, w.label, w.count);
        hipLaunchKernelGGL(clean_apply_kernel, dim3(vblocks), dim3(MC_THREADS), 0, stream, n,
            w.cut, w.referenced, w.label, w.count,
            (uint32_t)(opt.component_size > 1 ? opt.component_size : 1), opt.keep_unreferenced,
            w.counts, w.size, w.cut, w.vscan);
        SMVS_HIP_CHECK(hipGetLastError());
        if (int const rc = exclusive_scan(stream, w.vscan, n, w.vtiles); rc != SMVS_OK)
            return rc;
        hipLaunchKernelGGL(clean_compact_kernel, dim3(vblocks), dim3(MC_THREADS), 0, stream, n,
            w.cut, w.vscan, src, src_cells, dst, dst_cells);
    }
    if (n > 0 && m > 0) {
        hipLaunchKernelGGL(clean_face_keep_kernel, dim3(fblocks), dim3(MC_THREADS), 0, stream,
            src_faces, m, w.survive, w.vscan, w.fscan);
        SMVS_HIP_CHECK(hipGetLastError());
        if (int const rc = exclusive_scan(stream, w.fscan, m, w.ftiles); rc != SMVS_OK)
            return rc;
        hipLaunchKernelGGL(clean_face_compact_kernel, dim3(fblocks), dim3(MC_THREADS), 0, stream,
            src_faces, m, w.survive, w.fscan, w.vscan, dst_faces);
    }
    hipLaunchKernelGGL(clean_totals_kernel, dim3(1), dim3(1), 0, stream, w.counts,
        n > 0 ? scan_total(w.vtiles, n) : nullptr,
        n > 0 && m > 0 ? scan_total(w.ftiles, m) : nullptr);
    SMVS_HIP_CHECK(hipGetLastError());
    return SMVS_OK;
}

} // namespace smvs_hip

using namespace smvs_hip;

extern "C" int
smvs_mesh_clean(int device, int64_t n, int64_t m, const float *xyz, const float *normals,
    const uint8_t *rgb, const float *confidence, const int64_t *cells, const uint32_t *faces,
    const smvs_mesh_clean_options *options, uint32_t *component, uint32_t *component_size,
    int64_t *new_id, smvs_mesh_clean_stats *stats, smvs_points **handle, int64_t *n_vertices,
    int64_t *n_faces)
{
    SMVS_REQUIRE(handle != nullptr, "no handle pointer");
    *handle = nullptr;
    SMVS_REQUIRE(options != nullptr, "no options");
    smvs_mesh_clean_options const &opt = *options;
    SMVS_REQUIRE(n >= 0 && n <= 0x7fffffffll && m >= 0 && m <= 0x7fffffffll,
        "smvs_mesh_clean: n and m must be in 0 .. 2^31 - 1");
    SMVS_REQUIRE(std::isfinite(opt.threshold), "smvs_mesh_clean: threshold must be finite");
    // (a NaN fails both comparisons)
    SMVS_REQUIRE(opt.percentile >= 0.0f && opt.percentile <= 100.0f,
        "smvs_mesh_clean: percentile must be in [0, 100]");
    SMVS_REQUIRE(opt.threshold == 0.0f || opt.percentile == 0.0f,
        "smvs_mesh_clean: threshold and percentile exclude each other");
    SMVS_REQUIRE(n == 0 || (xyz && normals && rgb && confidence),
        "smvs_mesh_clean: a vertex array is missing");
    SMVS_REQUIRE(m == 0 || faces != nullptr, "smvs_mesh_clean: no faces");
    size_t const nv = (size_t)n, nf = (size_t)m;
    for (size_t i = 0; i < 3 * nf; ++i)
        SMVS_REQUIRE(faces[i] < (uint64_t)n, "smvs_mesh_clean: a face holds a vertex id >= n");

    int rc;
    WorkspaceLease lease(device);
    if (lease.w == nullptr)
        return SMVS_ERR_HIP;
    Workspace &ws = *lease.w;
    Carver carve;
    MeshCleanPieces const pieces = carve_mesh_clean(carve, nv, nf, component_size != nullptr);
    size_t const xyz_at = carve(12 * nv), nrm_at = carve(12 * nv), rgb_at = carve(3 * nv),
        conf_at = carve(4 * nv), cells_at = carve(cells != nullptr ? 8 * nv : 0),
        faces_at = carve(12 * nf);
    Carver oc;
    size_t const oxyz_at = oc(12 * nv), onrm_at = oc(12 * nv), orgb_at = oc(3 * nv),
        oconf_at = oc(4 * nv), ocells_at = oc(cells != nullptr ? 8 * nv : 0),
        ofaces_at = oc(12 * nf);
    char *slab = nullptr, *outs = nullptr;
    if ((rc = ws.ensure(0, carve.total, &slab)) || (rc = ws.ensure(1, oc.total, &outs)))
        return rc;
    MeshCleanWork const work = mesh_clean_work(slab, pieces);
    VertexAttrs const src = { reinterpret_cast<float *>(slab + xyz_at),
        reinterpret_cast<float *>(slab + nrm_at), reinterpret_cast<uint8_t *>(slab + rgb_at),
        reinterpret_cast<float *>(slab + conf_at), nullptr };
    VertexAttrs const dst = { reinterpret_cast<float *>(outs + oxyz_at),
        reinterpret_cast<float *>(outs + onrm_at), reinterpret_cast<uint8_t *>(outs + orgb_at),
        reinterpret_cast<float *>(outs + oconf_at), nullptr };
    long long *const src_cells = cells != nullptr ? reinterpret_cast<long long *>(slab + cells_at)
                                                  : nullptr;
    long long *const dst_cells = cells != nullptr ? reinterpret_cast<long long *>(outs + ocells_at)
                                                  : nullptr;
    uint32_t *const src_faces = reinterpret_cast<uint32_t *>(slab + faces_at);
    uint32_t *const dst_faces = reinterpret_cast<uint32_t *>(outs + ofaces_at);
    if ((rc = ws.upload(src.xyz, xyz, 12 * nv)) || (rc = ws.upload(src.nrm, normals, 12 * nv))
        || (rc = ws.upload(src.rgb, rgb, 3 * nv)) || (rc = ws.upload(src.conf, confidence, 4 * nv))
        || (cells != nullptr && (rc = ws.upload(src_cells, cells, 8 * nv)))
        || (rc = ws.upload(src_faces, faces, 12 * nf))
        || (rc = launch_mesh_clean(ws.stream, nv, nf, src, src_cells, src_faces, opt, work, dst,
                dst_cells, dst_faces)))
        return rc;
    MeshCleanCounts c;
    if ((rc = ws.download(&c, work.counts, sizeof(c))))
        return rc;
    smvs_points *h = nullptr;
    if ((rc = fill_points(ws, true, cells != nullptr, (size_t)c.n_vertices, (size_t)c.n_faces, dst,
            dst_faces, dst_cells, &h)))
        return rc;
    if ((component != nullptr && (rc = ws.download(component, work.label, 4 * nv)))
        || (component_size != nullptr && (rc = ws.download(component_size, work.size, 4 * nv)))
        || (new_id != nullptr && (rc = ws.download(new_id, work.vscan, 8 * nv)))) {
        delete h;
        return rc;
    }
    if (stats != nullptr) {
        stats->cut_value = c.cut_value;
        stats->n_cut = (int64_t)c.n_cut;
        stats->n_components = (int64_t)c.n_components;
        stats->n_small_components = (int64_t)c.n_small_components;
        stats->n_small_vertices = (int64_t)c.n_small_vertices;
        stats->n_unreferenced = (int64_t)c.n_unreferenced;
        stats->largest_component = (int64_t)c.largest_component;
    }
    *handle = h;
    if (n_vertices != nullptr)
        *n_vertices = h->n_points;
    if (n_faces != nullptr)
        *n_faces = h->n_faces;
    return SMVS_OK;
}

extern "C" int
smvs_mesh_clean_handle(int device, const smvs_points *in,
    const smvs_mesh_clean_options *options, uint32_t *component, uint32_t *component_size,
    int64_t *new_id, smvs_mesh_clean_stats *stats, smvs_points **handle, int64_t *n_vertices,
    int64_t *n_faces)
{
    SMVS_REQUIRE(handle != nullptr, "no handle pointer");
    *handle = nullptr;
    SMVS_REQUIRE(in != nullptr, "no handle");
    SMVS_REQUIRE(in->mesh || !in->faces.empty(), "smvs_mesh_clean_handle: the handle has no faces");
    return smvs_mesh_clean(device, in->n_points, in->n_faces, in->xyz.data(), in->nrm.data(),
        in->rgb.data(), in->conf.data(), in->sparse ? in->cells.data() : nullptr,
        in->faces.data(), options, component, component_size, new_id, stats, handle, n_vertices,
        n_faces);
}
