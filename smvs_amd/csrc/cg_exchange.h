// What crosses workgroups in the resident PCG (cg_resident.hip): the exchange
// area, tagged granule / pair stores and loads, the sums inside a workgroup and
// the two grid-wide all-reduces.  A fragment of cg_resident.hip's translation
// unit; nothing outside the kernel uses it.
#pragma once

#include "cg_resident_plan.h"
#include "dpp.h"

namespace smvs_hip {

constexpr int RES_WAVES = RES_THREADS / 64;

// Exchange area.  Zeroed when it is allocated, when the 15-bit solve id starts
// over and after a solve that gave up -- NOT before every launch: every tag
// carries the solve id (solve_tag | epoch), so what earlier solves left behind
// never matches.  A double travels as two 8-byte granules {tag, 32 data bits}:
// the data is its own flag (cdna_hip_programming.md Guideline 16, form R2), so
// one sweep over the granules of all workgroups is barrier and all-reduce at
// once.
constexpr int RES_KINDS = 8;                 // doubles per all-reduce, at most
constexpr int RES_GROUP = 16;                                  // workgroups per first-level group
constexpr int RES_MAX_GROUPS = RES_MAX_BLOCKS / RES_GROUP;
constexpr int RES_REPLICAS = 16;                               // copies of the group sums
constexpr int RES_DIRECT_GROUPS = 5;     // direct gather: groups per sweeping lane, at most
// ... and up to how many groups a grid gathers directly by default (measured,
// profiles/cg_direct_gather.txt)
constexpr int RES_DIRECT_GROUPS_DEFAULT = 5;
struct ResExchange {
    // flat all-reduce (two-exchange solver): every workgroup sweeps all of these
    unsigned long long gran[2][2 * RES_KINDS][RES_MAX_BLOCKS];   // [parity][..][wg]
    // tree all-reduce (one-exchange solver): a double is the pair {lo, hi} of
    // adjacent granules; the first workgroup of a group of RES_GROUP sums its
    // group's partial sums into lvl2, every workgroup sums the groups
    unsigned long long lvl1[2][RES_MAX_BLOCKS][RES_KINDS][2];    // [parity][wg][kind]
    // (RES_REPLICAS copies of the group sums, 2 KB apart: all 256 workgroups
    // polling the same sixteen cache lines made those lines' memory channel the
    // clock of the second hop -- a poll round there took as long as the channel
    // needed for 4,096 line reads, and a group's store queued behind them)
    unsigned long long lvl2[2][RES_REPLICAS][RES_MAX_GROUPS][RES_KINDS][2];   // [parity][copy][group][kind]
    unsigned timeout;
    // compacted solve: solve tag | 1 (the tile has an active node) or | 2 (it has
    // none: its workgroup has left), written once per solve by every workgroup
    unsigned live[RES_MAX_BLOCKS];
};

// Who takes part in an exchange (the compacted solve, see the kernel): the
// first LIVE workgroup of a group sums the group, members and groups without an
// active node are not waited for -- their sums are exactly +0.0, so leaving
// them out of the tree changes no bit of any total.
struct LiveSet {
    bool leads;         // this workgroup sums its group (wave-uniform)
    unsigned bits;      // lane (kind, j): bit 0 member j of its group is live, bit 1 group j is,
                        // bit 2 + g member j of group g < RES_DIRECT_GROUPS is (direct gather)
};

__device__ __forceinline__ void
st_agent(double *p, double v)
{
    __hip_atomic_store(reinterpret_cast<unsigned long long *>(p),
        (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED,
        __HIP_MEMORY_SCOPE_AGENT);
}

// Workgroup barrier that orders LDS traffic only.  __syncthreads() is also a
// release fence at workgroup scope: s_waitcnt vmcnt(0) in front of the
// s_barrier, so every wave that had published rim values sat at the next
// barrier until the fabric had acknowledged its write-through stores -- 2 to
// 2.8 us in EVERY iteration of the one-exchange solver (cg_trace.py, "sweep
// wave starts"; profiles/r4_cg_barrier.txt).  Nothing in this kernel passes
// data between the threads of a workgroup through global memory: what
// crosses workgroups carries its own tag, everything else is LDS.
__device__ __forceinline__ void
lds_barrier(void)
{
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// A double that crosses workgroups travels as two 8-byte granules {tag, 32
// data bits} (Guideline 16, form R2): the reader polls until both tags carry
// the value it expects, no release / drain on the writer's side.
__device__ __forceinline__ void
st_granules(unsigned long long *g, unsigned tag, double v)
{
    unsigned long long const bits = (unsigned long long)__double_as_longlong(v);
    __hip_atomic_store(g, ((unsigned long long)tag << 32) | (bits & 0xFFFFFFFFull),
        __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(g + 1, ((unsigned long long)tag << 32) | (bits >> 32),
        __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ double
ld_agent(const double *p)
{
    unsigned long long const v = __hip_atomic_load(
        reinterpret_cast<const unsigned long long *>(p), __ATOMIC_RELAXED,
        __HIP_MEMORY_SCOPE_AGENT);
    return __longlong_as_double((long long)v);
}

// Cross-lane sums without the LDS pipe.  __shfl_xor of a double is two
// ds_bpermute_b32, and the CU has ONE LDS unit for its eight waves: the eight
// butterflies of an exchange (8 kinds x 6 steps x 2 words x 8 waves = 768
// bpermutes) kept it busy for ~2.5 us per iteration -- the largest single item
// of an iteration, found with the per-wave stamps of tools/cg_trace.py
// (profiles/r4_cg_waves.txt).  gfx950 has what is needed on the VALU:
// v_permlane32_swap / v_permlane16_swap exchange halves / rows between two
// registers, DPP row rotations cover the 16 lanes of a row.
// (the moves themselves: dpp.h)

// HALF = 32: on return the lower 32 lanes hold x[l] + x[l + 32], the upper 32
// lanes y[l - 32] + y[l] -- one step of a reduce-scatter over two kinds (with
// y = x: a butterfly step).  HALF = 16: the same between the even and the odd
// rows of 16 lanes.  Every pair is summed as (lower lane) + (upper lane).
template <int HALF>
__device__ __forceinline__ double
swap_add(double x, double y)
{
    double lower, upper;
    permlane_swap_f64<HALF>(x, y, lower, upper);
    return lower + upper;
}

template <int ROR>
__device__ __forceinline__ double
row_rotated(double v)
{
    return dpp_f64<dpp_row_ror(ROR)>(v);
}

// Sum over the 16 lanes of a row, every lane gets it (bit-identical in all of
// them: after the rotation by 8 the values have period 8, so the two lanes of
// every later pair add the same two numbers).
__device__ __forceinline__ double
row_sum(double v)
{
    v += row_rotated<8>(v);
    v += row_rotated<4>(v);
    v += row_rotated<2>(v);
    v += row_rotated<1>(v);
    return v;
}

// First half of a workgroup sum of K per-thread values: the per-wave sums go
// to red[K][RES_WAVES]; after the barrier inside, the sum of kind k is
// red[k][0] + ... + red[k][RES_WAVES - 1] in that order (block_total).  The
// wave sums are a reduce-scatter: across the halves of the wave a lane keeps
// half of its kinds, across the rows of a half a quarter; what is left (two
// kinds of eight) is summed over the row.  Fixed order, the same in every wave
// and workgroup.
template <int K>
__device__ __forceinline__ void
wave_partials(double const (&v)[K], double *red /*[K][RES_WAVES]*/)
{
    constexpr int P = K <= 1 ? 1 : K <= 2 ? 2 : K <= 4 ? 4 : 8;   // kinds, padded
    static_assert(K <= 8, "block_partials: at most eight kinds");
    int const lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double a[P];
#pragma unroll
    for (int i = 0; i < P; ++i)
        a[i] = i < K ? v[i] : 0.0;
    // halves of the wave
    constexpr int N1 = P > 1 ? P / 2 : 1;
#pragma unroll
    for (int i = 0; i < N1; ++i)
        a[i] = swap_add<32>(a[i], P > 1 ? a[i + N1] : a[i]);
    // rows of a half
    constexpr int N2 = N1 > 1 ? N1 / 2 : 1;
#pragma unroll
    for (int i = 0; i < N2; ++i)
        a[i] = swap_add<16>(a[i], N1 > 1 ? a[i + N2] : a[i]);
#pragma unroll
    for (int i = 0; i < N2; ++i)
        a[i] = row_sum(a[i]);
    // which kinds this lane's row holds: bit 5 of the lane chose among the
    // halves of a[0 .. P), bit 4 among the halves of what was left
    int const b5 = lane >> 5, b4 = (lane >> 4) & 1;
    int const first = (P > 1 ? b5 * N1 : 0) + (N1 > 1 ? b4 * N2 : 0);
    if ((lane & 15) == 0 && (P > 1 || b5 == 0) && (N1 > 1 || b4 == 0)) {
#pragma unroll
        for (int i = 0; i < N2; ++i)
            if (first + i < K)
                red[(first + i) * RES_WAVES + wave] = a[i];
    }
}

template <int K>
__device__ __forceinline__ void
block_partials(double const (&v)[K], double *red /*[K][RES_WAVES]*/)
{
    wave_partials<K>(v, red);
    lds_barrier();
    // (no second barrier: the partials are next written by the following
    // block_partials, and every thread passes the caller's barrier behind the
    // sweep first)
}

// The same without the workgroup barrier: every wave raises its own tag behind
// its partial sums (LDS serves a wave's requests in order), and only the waves
// that need the workgroup's sums wait for the eight tags -- the others go on
// to their stores and polls.  The slots are safe to reuse: whoever reads them
// does so before the barrier at the end of the exchange, and they are written
// again only behind it.
struct PartialTags {
    volatile unsigned *tag;     // [RES_WAVES]
    __device__ __forceinline__ void raise(unsigned t) const
    {
        if ((threadIdx.x & 63) == 0) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            tag[threadIdx.x >> 6] = t;
        }
    }
    // wave-uniform; false after a bounded wait
    __device__ __forceinline__ bool wait(unsigned t) const
    {
        for (unsigned spins = 0; !__all(tag[threadIdx.x & (RES_WAVES - 1)] == t); ++spins) {
            if (spins > (1u << 22))
                return false;
            __builtin_amdgcn_s_sleep(1);
        }
        return true;
    }
};

__device__ __forceinline__ double
block_total(const double *red, int k)
{
    double s = 0.0;
#pragma unroll
    for (int wv = 0; wv < RES_WAVES; ++wv)
        s += red[k * RES_WAVES + wv];
    return s;
}

struct NoIdleWork {
    __device__ __forceinline__ void operator()() const {}
};

// All-reduce of K doubles over the workgroups of the grid, and the grid-wide
// synchronisation point of the phase: every workgroup publishes its K sums as
// tagged granules; K waves of every workgroup (kind k each, waves FIRST ..
// FIRST + K - 1) sweep the granules of all workgroups until every tag carries
// this epoch, then all sum them in the same fixed order.  The slots are
// double-buffered by epoch parity: a workgroup can publish epoch e + 2 only
// after everybody published e + 1, i.e. after everybody finished reading e.
// The waves that do not sweep run `idle` meanwhile (the halo of the
// one-exchange solver).  Returns false after a bounded wait (a workgroup is
// not resident / gave up).
template <int K, int FIRST, typename Idle>
__device__ __forceinline__ bool
grid_allreduce(ResExchange *ex, unsigned solve_tag, unsigned epoch, int nblocks,
    double (&v)[K], double *red, int *lds_flag, Idle idle)
{
    static_assert(K <= RES_KINDS && FIRST + K <= RES_WAVES, "sweeping waves");
    // tags carry the solve id: granules of earlier solves never match, so the
    // exchange area needs no clearing between solves
    unsigned const tag = solve_tag | epoch;
    double *res = red + RES_KINDS * RES_WAVES;   // [K] results, behind the partial sums
    block_partials<K>(v, red);
    if (nblocks == 1) {
        // a grid of one tile (the coarse scales, the tiny systems of the fuzz
        // sweep): nothing to exchange -- the workgroup's sums are the totals,
        // no granule leaves the CU (6 us per iteration on a loaded chip)
#pragma unroll
        for (int k = 0; k < K; ++k)
            v[k] = block_total(red, k);
        lds_barrier();   // (the partial sums are free for the next reduction)
        return true;
    }
    // (nothing to drain: everything that crosses workgroups is a granule, the
    // vectors of the solve live in registers and LDS)
    unsigned const par = epoch & 1u;
    if (threadIdx.x < 2 * K) {
        // (only the publishing threads need the workgroup's sums)
        int const k = threadIdx.x >> 1, half = threadIdx.x & 1;
        unsigned long long const bits = (unsigned long long)__double_as_longlong(
            block_total(red, k));
        unsigned const word = half ? (unsigned)(bits >> 32) : (unsigned)bits;
        __hip_atomic_store(&ex->gran[par][threadIdx.x][blockIdx.x],
            ((unsigned long long)tag << 32) | word, __ATOMIC_RELAXED,
            __HIP_MEMORY_SCOPE_AGENT);
    }
    int const wave = (int)(threadIdx.x >> 6) - FIRST;
    if (wave >= 0 && wave < K) {
        int const lane = threadIdx.x & 63;
        constexpr int PER_LANE = RES_MAX_BLOCKS / 64;
        unsigned lo[PER_LANE], hi[PER_LANE];
        bool ok = true;
        for (unsigned spins = 0;; ++spins) {
            bool all = true;
#pragma unroll
            for (int j = 0; j < PER_LANE; ++j) {
                int const blk = lane + 64 * j;
                unsigned long long g0 = (unsigned long long)tag << 32, g1 = g0;
                if (blk < nblocks) {
                    g0 = __hip_atomic_load(&ex->gran[par][2 * wave][blk],
                        __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    g1 = __hip_atomic_load(&ex->gran[par][2 * wave + 1][blk],
                        __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                lo[j] = (unsigned)g0;
                hi[j] = (unsigned)g1;
                all &= (unsigned)(g0 >> 32) == tag && (unsigned)(g1 >> 32) == tag;
            }
            if (__all(all))
                break;
            if (spins > (1u << 18)
                || ((spins & 255u) == 255u
                    && __hip_atomic_load(&ex->timeout, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT) != 0u)) {
                __hip_atomic_store(&ex->timeout, 1u, __ATOMIC_RELAXED,
                    __HIP_MEMORY_SCOPE_AGENT);
                ok = false;
                break;
            }
            __builtin_amdgcn_s_sleep(1);
        }
        // fixed order: workgroups lane, lane + 64, ... per lane, then the tree
        double sum = 0.0;
#pragma unroll
        for (int j = 0; j < PER_LANE; ++j) {
            unsigned long long const bits = ((unsigned long long)hi[j] << 32) | lo[j];
            sum += (lane + 64 * j) < nblocks
                ? __longlong_as_double((long long)bits) : 0.0;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1)
            sum += __shfl_xor(sum, off);
        if (lane == 0) {
            res[wave] = sum;
            // (a halo wait that gave up raises the same flag)
            if (wave == 0 && __hip_atomic_load(&ex->timeout, __ATOMIC_RELAXED,
                    __HIP_MEMORY_SCOPE_AGENT) != 0u)
                ok = false;
            lds_flag[wave] = ok ? 1 : 0;
        }
    } else {
        idle();
    }
    lds_barrier();
    // The results live apart from the partial sums, so two workgroup barriers
    // per all-reduce are enough (one inside block_partials, this one): results and
    // flags are next written behind the next all-reduce's first barrier, which
    // every thread reaches only after it has read these.
    bool ok = true;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        v[k] = res[k];
        ok = ok && lds_flag[k] != 0;
    }
    return ok;
}

// A double as ONE 16-byte write-through store / ONE 16-byte L1-bypassing load
// of its two adjacent granules {data lo, tag}, {data hi, tag}.  Both halves
// carry the tag, so nothing depends on the 16 bytes arriving together; what
// the wide access buys is half the number of fabric transactions of the
// exchange (an 8-byte sc1 store is one fabric write per lane:
// MI355X_MICROARCH.md, "stores of each flavour").
typedef unsigned int uint4_r __attribute__((ext_vector_type(4)));
constexpr int AUX_SC1 = 16;

__device__ __forceinline__ __amdgpu_buffer_rsrc_t
pair_buffer(void *base, size_t bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(base, 0, (int)bytes, 0x00020000);
}

__device__ __forceinline__ void
st_pair16(__amdgpu_buffer_rsrc_t buf, unsigned byte_offset, unsigned tag, double v)
{
    unsigned long long const bits = (unsigned long long)__double_as_longlong(v);
    uint4_r const w = { (unsigned)bits, tag, (unsigned)(bits >> 32), tag };
    __builtin_amdgcn_raw_buffer_store_b128(w, buf, (int)byte_offset, 0, AUX_SC1);
}

__device__ __forceinline__ bool
ld_pair16(__amdgpu_buffer_rsrc_t buf, unsigned byte_offset, unsigned tag, double *v)
{
    uint4_r const w = __builtin_amdgcn_raw_buffer_load_b128(buf, (int)byte_offset, 0,
        AUX_SC1);
    *v = __longlong_as_double((long long)(((unsigned long long)w.z << 32) | w.x));
    return w.y == tag && w.w == tag;
}

// The four doubles of one node's exchanged vector (64 bytes): four 16-byte
// loads per poll until all carry `want`; false after a bounded wait.
__device__ __forceinline__ void
nap(int units)
{
    for (int i = 0; i < units; ++i)
        __builtin_amdgcn_s_sleep(8);
}

__device__ __forceinline__ bool
poll_node_pairs(__amdgpu_buffer_rsrc_t buf, unsigned byte_offset, unsigned want,
    ResExchange *ex, double (&out)[4], int gap = 0)
{
    for (unsigned spins = 0;; ++spins) {
        bool ok = true;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            ok &= ld_pair16(buf, byte_offset + (unsigned)q * 16u, want, &out[q]);
        if (ok)
            return true;
        if (spins > (1u << 18)
            || ((spins & 255u) == 255u
                && __hip_atomic_load(&ex->timeout, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT) != 0u)) {
            __hip_atomic_store(&ex->timeout, 1u, __ATOMIC_RELAXED,
                __HIP_MEMORY_SCOPE_AGENT);
            return false;
        }
        __builtin_amdgcn_s_sleep(1);
        nap(gap);
        asm volatile("" ::: "memory");   // (the loads are re-issued every round)
    }
}

// One double as a pair of adjacent tagged granules: every lane of the wave
// polls its own pair (one 16-byte load) until all lanes see their tag
// (inactive lanes take no part and get 0).  Wave-uniform result: false after a
// bounded wait.
__device__ __forceinline__ bool
poll_pairs(__amdgpu_buffer_rsrc_t buf, unsigned byte_offset, bool active, unsigned tag,
    ResExchange *ex, double *value, int gap = 0, unsigned *rounds = nullptr)
{
    double got = 0.0;
    bool mine_ok = !active;
    bool good = true;
    for (unsigned spins = 0;; ++spins) {
        if (!mine_ok)
            mine_ok = ld_pair16(buf, byte_offset, tag, &got);
        if (__all(mine_ok))
            break;
        if (rounds != nullptr)
            *rounds += 1;
        if (spins > (1u << 18)
            || ((spins & 255u) == 255u
                && __hip_atomic_load(&ex->timeout, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT) != 0u)) {
            __hip_atomic_store(&ex->timeout, 1u, __ATOMIC_RELAXED,
                __HIP_MEMORY_SCOPE_AGENT);
            good = false;
            break;
        }
        __builtin_amdgcn_s_sleep(1);
        nap(gap);
        asm volatile("" ::: "memory");
    }
    *value = active ? got : 0.0;
    if (rounds != nullptr)
        *rounds += 1;
    return good;
}

// The direct gather's poll: lane (kind, j) waits for member j of each of G
// groups, `stride` bytes apart (bit g of `active`: that member takes part),
// with all its outstanding pairs in flight at once; a pair that has arrived is
// not loaded again.  Members that take no part give 0.  Wave-uniform result:
// false after a bounded wait.
template <int G>
__device__ __forceinline__ bool
poll_group_pairs(__amdgpu_buffer_rsrc_t buf, unsigned byte_offset, unsigned stride,
    unsigned active, unsigned tag, ResExchange *ex, double (&value)[G], int gap = 0,
    unsigned *rounds = nullptr)
{
    // (the pairs stay in the registers they were loaded into: the kernel has
    // none to spare)
    uint4_r w[G];
#pragma unroll
    for (int g = 0; g < G; ++g)
        w[g] = (uint4_r){ 0u, 0u, 0u, 0u };
    unsigned pending = active;
    bool good = true;
    for (unsigned spins = 0;; ++spins) {
#pragma unroll
        for (int g = 0; g < G; ++g)
            if ((pending >> g) & 1u)
                w[g] = __builtin_amdgcn_raw_buffer_load_b128(buf, (int)byte_offset,
                    (int)((unsigned)g * stride), AUX_SC1);
#pragma unroll
        for (int g = 0; g < G; ++g)
            if (w[g].y == tag && w[g].w == tag)
                pending &= ~(1u << g);
        if (__all(pending == 0u))
            break;
        if (rounds != nullptr)
            *rounds += 1;
        if (spins > (1u << 18)
            || ((spins & 255u) == 255u
                && __hip_atomic_load(&ex->timeout, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT) != 0u)) {
            __hip_atomic_store(&ex->timeout, 1u, __ATOMIC_RELAXED,
                __HIP_MEMORY_SCOPE_AGENT);
            good = false;
            break;
        }
        __builtin_amdgcn_s_sleep(1);
        nap(gap);
        asm volatile("" ::: "memory");
    }
#pragma unroll
    for (int g = 0; g < G; ++g)
        value[g] = ((active >> g) & 1u)
            ? __longlong_as_double((long long)(((unsigned long long)w[g].z << 32) | w[g].x))
            : 0.0;
    if (rounds != nullptr)
        *rounds += 1;
    return good;
}

// Sum over the 16 / 32 lanes of an aligned segment, fixed order, every lane gets it.
__device__ __forceinline__ double
segment16_sum(double v)
{
    return row_sum(v);
}

__device__ __forceinline__ double
segment32_sum(double v)
{
    return row_sum(swap_add<16>(v, v));
}

// Who publishes the sums of an exchange.  On gfx9 loads and stores share ONE
// counter (vmcnt): a wave that has issued a write-through store cannot see the
// result of a later load before the fabric has acknowledged that store.  The
// sweeping waves live on their polls, so the workgroup's sums -- and, in a
// group's first workgroup, the group's sums, which the sweeping waves hand
// over through LDS -- are stored by the last wave, which never waits for a
// load.  (The rim's q is published by the owners of the nodes: one wave
// issuing all ~380 write-through stores of a tile was measured and is far
// slower, the issue rate of such stores is what counts there.)
// (the wave of the middle rows of a tile: the fewest rim nodes, so the fewest
// write-through stores of its own in front of the sums)
constexpr int RES_SUM_WAVE = 5;

// LDS mailbox between the sweeping waves and the publishing wave of a group's
// first workgroup: value first, then the tag (LDS serves a wave's requests in
// order), read in the opposite order.
struct GroupMailbox {
    volatile double *value;     // [RES_KINDS]
    volatile unsigned *tag;     // [RES_KINDS]
    __device__ __forceinline__ void put(int kind, unsigned t, double v) const
    {
        value[kind] = v;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        tag[kind] = t;
    }
    // (one lane per kind) false after a bounded wait
    __device__ __forceinline__ bool take(int kind, unsigned t, double *v) const
    {
        for (unsigned spins = 0; tag[kind] != t; ++spins) {
            if (spins > (1u << 22))
                return false;
            __builtin_amdgcn_s_sleep(1);
        }
        *v = value[kind];
        return true;
    }
};

__device__ __forceinline__ GroupMailbox
group_mailbox(double *red)
{
    double *base = red + RES_KINDS * RES_WAVES + RES_KINDS + (RES_KINDS + 1) / 2;
    return { base, reinterpret_cast<volatile unsigned *>(base + RES_KINDS) };
}

__device__ __forceinline__ PartialTags
partial_tags(double *red)
{
    double *base = red + RES_KINDS * RES_WAVES + RES_KINDS + (RES_KINDS + 1) / 2
        + RES_KINDS + (RES_KINDS + 1) / 2;
    return { reinterpret_cast<volatile unsigned *>(base) };
}

// All-reduce of K doubles over the workgroups in two levels.  The flat sweep
// above makes every workgroup read every workgroup's K sums: 256 x 256 x K
// granule pairs per exchange, all aimed at the same few KB -- measured, its
// time grows with K (4.4 us for one sum, 6.2 for three, 12 for seven).  Here
// the first workgroup of every group of RES_GROUP sums its group (16 x K
// pairs), publishes the group's sums, and every workgroup sums the <= 16
// groups: 2 x 16 x K pairs per workgroup and exchange instead of 256 x K, two
// hops instead of one.  Lane (kind, j) of the sweeping waves 1 .. (K + 3) / 4
// handles member / group j of one kind; the other waves run `others(wave)`.
// Same guarantees as the flat form: fixed summation order (a tree over the
// members of a group, then a tree over the groups), bit-identical results in
// every workgroup, slots double-buffered by epoch parity, bounded waits.
//
// The direct gather (DIRECT: 1 < ngroups <= RES_DIRECT_GROUPS, the same in
// every workgroup of a launch: the host chooses by nblocks alone).  The same
// tree in ONE hop: nobody leads, nothing goes to lvl2 or through the mailbox;
// lane (kind, j) of every workgroup polls member j of EVERY group, all pairs
// in flight at once -- 75 x K pairs per workgroup at 75 tiles, no dependent
// second hand-off across CUs (6.4 instead of 7.1 us per iteration there).  The totals keep the bits of the two-level form:
// part_g = segment16_sum(members of group g) is what group g's leader computes,
// on the same lane positions; every lane of the segment holds every part_g, lane
// j keeps part_j (0.0 for j >= ngroups) and the segment runs segment16_sum
// again: the tree over the groups on the lanes the second hop uses.  A group
// that is wholly dead gives segment16_sum of zeros = +0.0 where the second hop
// takes a literal 0.0 for the lane it does not poll: the same bits.
// Slot reuse with every workgroup as reader of every lvl1 slot: a workgroup
// publishes epoch e + 2 only after it has the totals of e + 1; those exist only
// after every workgroup published e + 1; and every workgroup published e + 1
// only after it had finished reading e (its sweepers' values are in res[]
// behind the barrier that ends e).  So nobody still reads the slot of parity e
// when e + 2 is written into it.
// DIRECT is a compile-time choice (kernels of their own, see cg_resident.hip);
// the host launches such a kernel only on grids of at most RES_DIRECT_GROUPS
// groups.
template <int K, bool DIRECT, typename Others, typename Mark>
__device__ __forceinline__ bool
grid_allreduce_tree(ResExchange *ex, unsigned solve_tag, unsigned epoch, int nblocks,
    LiveSet const live, double (&v)[K], double *red, int *lds_flag, Others others, Mark mark,
    int wait_member = 6, int wait_poll = 0)
{
    constexpr int SWEEPERS = (K + 3) / 4;
    static_assert(K <= RES_KINDS && 1 + SWEEPERS <= RES_SUM_WAVE, "sweeping waves");
    unsigned const tag = solve_tag | epoch;
    double *res = red + RES_KINDS * RES_WAVES;
    GroupMailbox const box = group_mailbox(red);
    PartialTags const partials = partial_tags(red);
    wave_partials<K>(v, red);
    partials.raise(tag);
    mark(20, -1);
    unsigned const par = epoch & 1u;
    int const b = (int)blockIdx.x;
    __amdgpu_buffer_rsrc_t const xbuf = pair_buffer(ex, sizeof(ResExchange));
    auto lvl1_at = [&](int wg, int kind) {
        return (unsigned)(offsetof(ResExchange, lvl1)
            + ((((size_t)par * RES_MAX_BLOCKS + (size_t)wg) * RES_KINDS + (size_t)kind) * 16));
    };
    auto lvl2_at = [&](int copy, int group, int kind) {
        return (unsigned)(offsetof(ResExchange, lvl2)
            + (((((size_t)par * RES_REPLICAS + (size_t)copy) * RES_MAX_GROUPS + (size_t)group)
                   * RES_KINDS + (size_t)kind) * 16));
    };
    int const ngroups = (nblocks + RES_GROUP - 1) / RES_GROUP;
    bool const leads = !DIRECT && live.leads;
    bool const member_live = (live.bits & 1u) != 0u, group_live = (live.bits & 2u) != 0u;
    int const wave = (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (wave == RES_SUM_WAVE) {
        bool handed = partials.wait(tag);
        mark(21, -1);
        if (nblocks > 1 && lane < K)
            st_pair16(xbuf, lvl1_at(b, lane), tag, block_total(red, lane));
        if (leads) {
            // lane (copy, kind): eight copies per store instruction
            static_assert(K == 8, "eight kinds per copy");
            double part = 0.0;
            handed = box.take(lane & 7, tag, &part) && handed;
#pragma unroll
            for (int c = lane >> 3; c < RES_REPLICAS; c += 8)
                st_pair16(xbuf, lvl2_at(c, b / RES_GROUP, lane & 7), tag, part);
        }
        if (!__all(handed) && lane == 0)
            __hip_atomic_store(&ex->timeout, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        others(wave);
    } else if (wave >= 1 && wave <= SWEEPERS) {
        int const kind = 4 * (wave - 1) + (lane >> 4), j = lane & 15;
        bool const kind_ok = kind < K;
        bool ok = true, ok2 = true;
        double total;
        unsigned rounds1 = 0, rounds2 = 0;
        mark(8, -1);
        if (nblocks == 1) {
            // a grid of one tile (the coarse scales): nothing to exchange
            ok = partials.wait(tag);
            total = kind_ok ? block_total(red, kind) : 0.0;
        } else if (ngroups == 1) {
            // a single group: every workgroup sums its <= 16 members itself,
            // one hop instead of two
            ok = poll_pairs(xbuf, lvl1_at(j < nblocks ? j : 0, kind_ok ? kind : 0),
                kind_ok && j < nblocks && member_live, tag, ex, &total, wait_poll);
            total = segment16_sum(total);
        } else if constexpr (DIRECT) {
            // the direct gather: member j of every group, then both levels of
            // the tree on this segment
            unsigned active = 0u;
#pragma unroll
            for (int g = 0; g < RES_DIRECT_GROUPS; ++g)
                if (kind_ok && RES_GROUP * g + j < nblocks && ((live.bits >> (2 + g)) & 1u))
                    active |= 1u << g;
            double part[RES_DIRECT_GROUPS];
            ok = poll_group_pairs<RES_DIRECT_GROUPS>(xbuf, lvl1_at(j, kind_ok ? kind : 0),
                (unsigned)(RES_GROUP * RES_KINDS * 16), active, tag, ex, part, wait_poll,
                &rounds1);
            mark(5, -1);
            mark(9, -1);
            total = 0.0;
#pragma unroll
            for (int g = 0; g < RES_DIRECT_GROUPS; ++g) {
                double const sum_g = segment16_sum(part[g]);
                total = j == g && g < ngroups ? sum_g : total;
            }
            total = segment16_sum(total);
        } else {
            if (leads) {
                // this workgroup sums its group
                int const member = b - b % RES_GROUP + j;
                double part;
                ok = poll_pairs(xbuf, lvl1_at(member < nblocks ? member : b,
                        kind_ok ? kind : 0), kind_ok && member < nblocks && member_live, tag,
                    ex, &part, wait_poll, &rounds1);
                part = segment16_sum(part);
                mark(5, -1);
                if (kind_ok && j == 0)
                    box.put(kind, tag, part);
            } else {
                // the group sums cannot be there yet (they are a hop behind)
                nap(wait_member);
            }
            mark(9, -1);
            ok2 = poll_pairs(xbuf, lvl2_at(b % RES_REPLICAS, j < ngroups ? j : 0,
                    kind_ok ? kind : 0),
                kind_ok && j < ngroups && group_live, tag, ex, &total, wait_poll, &rounds2);
            total = segment16_sum(total);
        }
        mark(6, -1);
        mark(10, (long long)(rounds1 * 1000u + rounds2));
        if (kind_ok && j == 0)
            res[kind] = total;
        if (lane == 0) {
            bool flag_ok = ok && ok2;
            // (a wait of another wave that gave up raises the same flag)
            if (wave == 1 && __hip_atomic_load(&ex->timeout, __ATOMIC_RELAXED,
                    __HIP_MEMORY_SCOPE_AGENT) != 0u)
                flag_ok = false;
            lds_flag[wave - 1] = flag_ok ? 1 : 0;
        }
    } else {
        others(wave);
    }
    lds_barrier();
    bool ok = true;
#pragma unroll
    for (int k = 0; k < K; ++k)
        v[k] = res[k];
#pragma unroll
    for (int w = 0; w < SWEEPERS; ++w)
        ok = ok && lds_flag[w] != 0;
    return ok;
}

} // namespace smvs_hip
