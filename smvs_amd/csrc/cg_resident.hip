// Preconditioned conjugate gradient with the matrix resident on the chip.
//
// Same solver as cg.hip (ConjugateGradient::solve, lib/conjugate_gradient.h:72-202,
// on the block stencil of BlockSparseMatrix<4>), different data movement.  The
// streaming kernels of cg.hip read the matrix H (83 MB at 1920x1080, scale 2)
// once per iteration: 150 MB per iteration through L2 / Infinity Cache and two
// launches, ~33 us per iteration however small the active set is.  Here ONE
// launch runs the whole solve:
//
//   * the node grid is cut into <= 256 tiles of <= 512 nodes, one workgroup
//     (512 threads, one per node) per tile, one workgroup per CU;
//   * a thread keeps its node's five stored blocks (the diagonal one as its
//     10 unique entries + the four upper neighbours, 74 doubles = 148 VGPRs)
//     in REGISTERS for the whole solve: the 128 MB register file holds the
//     83 MB matrix, H is read from HBM once per solve instead of once per
//     iteration;
//   * the product uses the symmetry the storage already exploits: thread m
//     forms  B d  for its five blocks (its own rows) and  B^T d_m  for its four
//     upper blocks (the rows of the upper neighbours, handed over through
//     LDS); rows whose lower neighbour lives in another tile use a copy of
//     that neighbour's block kept in LDS (the tile's rim, 18 KB);
//   * what crosses workgroups is tagged data that is its own flag (16-byte
//     pairs {32 data bits, tag} x 2, write-through stores, L1-bypassing
//     loads, no fence): per iteration of the one-exchange solver the q of the
//     rim nodes for the neighbours' halo and eight partial sums per workgroup
//     for a two-level all-reduce; every workgroup sums in the same fixed order,
//     so all derive bit-identical alpha / beta and take the same branch;
//   * inside a workgroup the waves have roles during an exchange (wave 0 the
//     halo, waves 1.. the sums, wave 5 the stores of the sums), the cross-lane
//     sums run on the VALU (v_permlane*_swap, DPP) and the barriers order LDS
//     only -- each of the three for a measured reason, see there.
//
// Numerics: the same operations as the reference except the association of
// the sums (row sums collect the transposed contributions after the stored
// ones; dot products are tree sums, as in cg.hip).  Deterministic: the result
// does not depend on scheduling.  x, the iteration count and `info` are
// checked against the oracle by the same tests as the streaming solver.
//
// Every spin is bounded: if the workgroups are not all resident (another
// barrier kernel holds CUs, fewer CUs than tiles) the barrier times out, the
// solve reports failure and the caller falls back to the streaming kernels.
#include "newton_step.h"
#include "cg_resident_plan.h"
#include "cg_exchange.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>

namespace smvs_hip {

typedef double double4_r __attribute__((ext_vector_type(4)));

constexpr int RES_PIPELINED = 1;      // launch-ahead Newton loop (newton_loop.hip)
constexpr int RES_TEST_GIVE_UP = 2;   // report a failure (test hook)

struct ResArgs {
    const double *H9;        // [5][N][16]
    const double *Pinv;      // [N][16]
    const double *g;         // [N][4]
    double *x, *b;           // [N][4], touched by the owning thread only
    unsigned long long *zg;  // two-exchange solver: [N][4][2] z of the rim nodes as tagged
                             // granules; one-exchange solver: [2][N][4][2] q of the rim
                             // nodes as tagged pairs, double-buffered by iteration parity
    ResExchange *ex;
    CgState *state;          // [2] (state[0] is written at the end)
    int *status;
    int *progress;           // pinned host words (common.h, PROGRESS_*)
    int solve_tag;
    int num_nodes, stride, rows;
    int tw, th, tiles_x, num_tiles;
    int max_iterations;
    double q_tolerance, fixed_tolerance;
    long long *trace;        // debug: 100 MHz wall-clock stamps (or nullptr)
    int trace_wg;            // ... of this workgroup's iterations (SMVS_CG_TRACE_WG)
    int pipelined;           // RES_PIPELINED | RES_TEST_GIVE_UP
    // fused assembly (the Newton loop): per-patch systems instead of H / g / P
    const double *Hp;        // the packed per-patch systems, 36 quads per patch ...
    const double *gp;        // ... and gradients, 4 quads per patch, laid out as
    PatchLayout layout;      // this says (common.h)
    const uint8_t *patch_valid;
    const uint8_t *active;
    uint8_t *active_next;    // cleared for the node update of this step
    double *scalars;
    int npx, npy;
    const double *zeros;     // 16 doubles of +0.0 (a block that does not contribute)
    // polling cadence of the one-exchange solver (units of s_sleep(8) = 512
    // cycles ~ 0.25 us): before the halo's first poll, before a group
    // member's first poll of the group sums, between two polls
    int wait_halo, wait_member, wait_poll;
    int compact;             // leave out what has no active node (SMVS_CG_COMPACT, default 1)
};

} // namespace smvs_hip

#include "cg_resident_assemble.h"

namespace smvs_hip {

constexpr int TRACE_ITERS = 12, TRACE_POINTS = 12;
// after the iteration rows: four prologue stamps of every workgroup
constexpr int TRACE_BLOCK_BASE = (TRACE_ITERS + 1) * TRACE_POINTS;
// ... and four stamps of every workgroup in iteration TRACE_SKEW_ITER of the
// one-exchange solver (start, sums published, totals received, halo collected):
// how far apart the tiles run
constexpr int TRACE_SKEW_BASE = TRACE_BLOCK_BASE + 4 * RES_MAX_BLOCKS;
constexpr int TRACE_SKEW_ITER = 5;
// ... and eight stamps of every wave of workgroup SMVS_CG_TRACE_WG in the same iteration
constexpr int TRACE_WAVE_BASE = TRACE_SKEW_BASE + 4 * RES_MAX_BLOCKS;
constexpr int TRACE_TOTAL = TRACE_WAVE_BASE + 8 * 8;

// What tools/cg_trace.py reads: the stamps of one solve, appended to `path`.
static void
dump_trace(const char *path, const long long *tr, int num_nodes, int num_tiles,
    int iterations, int exchanges)
{
    FILE *f = std::fopen(path, "a");
    if (f == nullptr)
        return;
    std::fprintf(f, "solve nodes=%d tiles=%d its=%d exchanges=%d\n",
        num_nodes, num_tiles, iterations, exchanges);
    for (int k = 0; k <= TRACE_ITERS; ++k) {
        for (int q = 0; q < TRACE_POINTS; ++q)
            std::fprintf(f, "%lld ", tr[(size_t)k * TRACE_POINTS + q]);
        std::fprintf(f, "\n");
    }
    for (int b = 0; b < num_tiles; ++b)
        std::fprintf(f, "block %d %lld %lld %lld %lld\n", b,
            tr[TRACE_BLOCK_BASE + 4 * b], tr[TRACE_BLOCK_BASE + 4 * b + 1],
            tr[TRACE_BLOCK_BASE + 4 * b + 2], tr[TRACE_BLOCK_BASE + 4 * b + 3]);
    for (int w = 0; w < 8; ++w) {
        std::fprintf(f, "wave %d", w);
        for (int q = 0; q < 8; ++q)
            std::fprintf(f, " %lld", tr[TRACE_WAVE_BASE + 8 * w + q]);
        std::fprintf(f, "\n");
    }
    for (int b = 0; b < num_tiles; ++b)
        std::fprintf(f, "skew %d %lld %lld %lld %lld\n", b,
            tr[TRACE_SKEW_BASE + 4 * b], tr[TRACE_SKEW_BASE + 4 * b + 1],
            tr[TRACE_SKEW_BASE + 4 * b + 2], tr[TRACE_SKEW_BASE + 4 * b + 3]);
    std::fclose(f);
}

// Position of a thread in its tile and the addressing that follows from it.
struct TileGeom {
    int tw, th, LW, lx, ly, li, lcore;
    // index of the copy (in the tile's rim array) of the block that the lower
    // neighbour of slot s = 0..3 <-> (dx, dy) = (-1,-1), (0,-1), (1,-1), (-1,0)
    // stores towards this node
    __device__ __forceinline__ int rim_index(int s) const
    {
        int const dx = s == 3 ? -1 : s - 1, dy = s == 3 ? 0 : -1;
        if (ly + dy < 0)
            return s * tw + lx;
        if (lx + dx < 0)
            return 3 * tw + (s == 0 ? 0 : th) + ly;
        return 3 * tw + 2 * th + ly;
    }
};

// acc = (H d)_node for the thread's node: its five stored blocks on the
// direction tile (own rows), the transposed products of its four upper blocks
// handed to the upper neighbours through `yl` one direction at a time (within
// a direction every row receives exactly one contribution: no atomics, fixed
// order), and the rows whose lower neighbour belongs to another tile from the
// copies of that neighbour's blocks in `fb`.  dself = d of the node.  Four
// workgroup barriers; the caller has synchronised the direction tile.
__device__ __forceinline__ void
tile_product(TileGeom const &G, const double *dtile, double *yl, const double *fb,
    double const (&hd)[10], double const (&hu)[4][16], unsigned low, unsigned up,
    bool mine, double (&acc)[4], double (&dself)[4])
{
    int const LW = G.LW, lcore = G.lcore;
    const double4_r *dt = reinterpret_cast<const double4_r *>(dtile);
    {
        double4_r const ds = dt[lcore];
        dself[0] = ds.x; dself[1] = ds.y; dself[2] = ds.z; dself[3] = ds.w;
        {
            // diagonal block from its upper triangle
            double const *d4 = dself;
            acc[0] = hd[0] * d4[0] + hd[1] * d4[1] + hd[2] * d4[2] + hd[3] * d4[3];
            acc[1] = hd[1] * d4[0] + hd[4] * d4[1] + hd[5] * d4[2] + hd[6] * d4[3];
            acc[2] = hd[2] * d4[0] + hd[5] * d4[1] + hd[7] * d4[2] + hd[8] * d4[3];
            acc[3] = hd[3] * d4[0] + hd[6] * d4[1] + hd[8] * d4[2] + hd[9] * d4[3];
        }
#pragma unroll
        for (int s = 5; s < 9; ++s) {
            int const dx = s % 3 - 1, dy = s / 3 - 1;
            double4_r const dm = dt[lcore + dy * LW + dx];
            double const dv[4] = { dm.x, dm.y, dm.z, dm.w };
#pragma unroll
            for (int row = 0; row < 4; ++row)
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    acc[row] = __builtin_fma(hu[s - 5][row * 4 + c], dv[c],
                        acc[row]);
        }
    }
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        if ((up >> kk) & 1u) {
            int const s = 5 + kk;
            int const dx = s % 3 - 1, dy = s / 3 - 1;
            int const target = (G.ly + dy) * G.tw + G.lx + dx;
            double t[4] = { 0.0, 0.0, 0.0, 0.0 };
#pragma unroll
            for (int row = 0; row < 4; ++row)
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    t[c] = __builtin_fma(hu[kk][row * 4 + c], dself[row],
                        t[c]);
            double4_r *dst = reinterpret_cast<double4_r *>(
                yl + (size_t)target * 4);
            double4_r const cur = *dst;
            *dst = (double4_r){ cur.x + t[0], cur.y + t[1], cur.z + t[2],
                cur.w + t[3] };
        }
        lds_barrier();
    }
    if (mine) {
        {
            double4_r const cv = *reinterpret_cast<const double4_r *>(
                yl + (size_t)G.li * 4);
            acc[0] += cv.x; acc[1] += cv.y; acc[2] += cv.z; acc[3] += cv.w;
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            unsigned const kind = (low >> (2 * s)) & 3u;
            if (kind == 2u) {
                int const dx = s == 3 ? -1 : s - 1, dy = s == 3 ? 0 : -1;
                double4_r const dm = dt[lcore + dy * LW + dx];
                double const dv[4] = { dm.x, dm.y, dm.z, dm.w };
                const double4_r *blk = reinterpret_cast<const double4_r *>(
                    fb + (size_t)G.rim_index(s) * 16);
#pragma unroll
                for (int row = 0; row < 4; ++row) {
                    double4_r const br = blk[row];
                    acc[0] = __builtin_fma(br.x, dv[row], acc[0]);
                    acc[1] = __builtin_fma(br.y, dv[row], acc[1]);
                    acc[2] = __builtin_fma(br.z, dv[row], acc[2]);
                    acc[3] = __builtin_fma(br.w, dv[row], acc[3]);
                }
            }
        }
    }
}

// The symmetric 4 x 4 block of node `li` from its upper triangle in three
// planes (see resident_lds_layout).
__device__ __forceinline__ void
load_symmetric(const double *planes, int tile_nodes, int li, double (&P)[4][4])
{
    const double4_r *Pu = reinterpret_cast<const double4_r *>(planes);
    double4_r const a = Pu[li], b = Pu[tile_nodes + li], c = Pu[2 * tile_nodes + li];
    P[0][0] = a.x; P[0][1] = a.y; P[0][2] = a.z; P[0][3] = a.w;
    P[1][0] = a.y; P[1][1] = b.x; P[1][2] = b.y; P[1][3] = b.z;
    P[2][0] = a.z; P[2][1] = b.y; P[2][2] = b.w; P[2][3] = c.x;
    P[3][0] = a.w; P[3][1] = b.z; P[3][2] = c.x; P[3][3] = c.y;
}

// z = P r with the reference's operation order (block_sparse_matrix.h:276-298
// on a diagonal block: products added one by one, no contraction)
__device__ __forceinline__ void
precondition(double const (&P)[16], double const (&r)[4], double (&z)[4])
{
#pragma clang fp contract(off)
#pragma unroll
    for (int row = 0; row < 4; ++row) {
        double zi = 0.0;
        zi += P[row * 4 + 0] * r[0];
        zi += P[row * 4 + 1] * r[1];
        zi += P[row * 4 + 2] * r[2];
        zi += P[row * 4 + 3] * r[3];
        z[row] = zi;
    }
}

// Polls the eight granules of one node's exchanged vector until all carry
// `want`; false after a bounded wait (the exchange's timeout flag is raised).
__device__ __forceinline__ bool
poll_node_granules(const unsigned long long *src, unsigned want, ResExchange *ex,
    double (&out)[4])
{
    for (unsigned spins = 0;; ++spins) {
        unsigned long long g[8];
        bool ok = true;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            g[q] = __hip_atomic_load(src + q, __ATOMIC_RELAXED,
                __HIP_MEMORY_SCOPE_AGENT);
            ok &= (unsigned)(g[q] >> 32) == want;
        }
        if (ok) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                out[q] = __longlong_as_double((long long)(
                    (g[2 * q + 1] << 32) | (g[2 * q] & 0xFFFFFFFFull)));
            return true;
        }
        if (spins > (1u << 18)) {
            __hip_atomic_store(&ex->timeout, 1u, __ATOMIC_RELAXED,
                __HIP_MEMORY_SCOPE_AGENT);
            return false;
        }
        __builtin_amdgcn_s_sleep(1);
    }
}

// LDS carve (doubles) of the two solver variants; the host sizes the launch
// with the same function.
struct ResLds {
    size_t dtile, yl, Pl, rl, fb, xl, bl, rh, Ph, qh, hinfo, red, live, total;
};
__host__ __device__ __forceinline__ ResLds
resident_lds_layout(int tw, int th, bool one)
{
    size_t const tn = (size_t)tw * th;
    size_t const ring = (size_t)2 * (tw + 2) + 2 * th;
    ResLds L;
    size_t o = 0;
    L.dtile = o; o += (size_t)(tw + 2) * (th + 2) * 4;   // direction tile with halo
    L.yl = o; o += tn * 4;                               // row sums from below
    // P: four row planes (two-exchange solver), or its upper triangle in three
    // planes {p00 p01 p02 p03} {p11 p12 p13 p22} {p23 p33 - -} (one-exchange
    // solver: ldl_inverse4 forms P[c1][c2] and P[c2][c1] from the same products
    // in the same order, so P is symmetric to the bit) -- the 16 KB saved hold
    // r there, which frees eight registers in a kernel that spills
    L.Pl = o; o += (one ? 3 : 4) * tn * 4;
    L.rl = o; o += one ? tn * 4 : 0;                     // r (one-exchange solver)
    L.fb = o; o += (size_t)(3 * tw + 3 * th) * 16;       // rim blocks
    L.xl = o; o += tn * 4;                               // x
    L.bl = o; o += one ? 0 : tn * 4;                     // b (two-exchange solver only)
    L.rh = o; o += one ? ring * 4 : 0;                   // r of the halo nodes
    L.Ph = o; o += one ? ring * 16 : 0;                  // P of the halo nodes
    L.qh = o; o += one ? ring * 4 : 0;                   // q of the halo nodes (one iteration)
    L.hinfo = o; o += one ? (ring + 1) / 2 : 0;          // per halo slot: node id (ints)
    L.red = o; o += RES_KINDS * RES_WAVES + RES_KINDS;   // partial sums + results
    o += (RES_KINDS + 1) / 2;                            // flags (ints)
    o += RES_KINDS + (RES_KINDS + 1) / 2;                // group mailbox: values, tags (ints)
    o += (RES_WAVES + 1) / 2;                            // tags of the waves' partial sums (ints)
    L.live = o; o += RES_MAX_BLOCKS / 64;                // which tiles have an active node (bits)
    L.total = o;
    return L;
}

// ONE = false: the reference's operation order -- d.Ad is reduced first, then
// r.r, x.(b + r), z.r of the updated vectors: two grid-wide exchanges per
// iteration (conjugate_gradient.h:121-198 line by line).
// ONE = true: one exchange per iteration.  Before the step length is known
// the workgroups reduce eight dot products of the CURRENT vectors,
//   d.q, r.q, q.q, 2 w.r, w.q, d.r, r.r, z.r    (q = H d, w = P q),
// from which alpha and the three scalars the reference tests follow exactly
// (no approximation, only the association of the sums changes):
//   r'.r'      = r.r - 2 alpha r.q + alpha^2 q.q          (r' = r - alpha q)
//   z'.r'      = z.r - 2 alpha w.r + alpha^2 w.q          (z' = P r' = z - alpha w;
//                                                          z.q = w.r, P symmetric)
//   x'.(b+r')  = x.(b+r) + 2 alpha d.r - alpha^2 d.q      (x' = x + alpha d,
//                                                          b - r = H x)
// r.r and z.r are summed directly in every iteration and only extrapolated
// ONE step (carried by recurrence over a whole solve, z.r kept the absolute
// rounding errors of its large early values while it shrank by orders of
// magnitude: iteration counts on ill-conditioned systems moved by up to 10 %).
// The vectors themselves are updated with the reference's operations (z = P r
// is recomputed, not taken from the recurrence).  The second grid-wide wait of
// an iteration -- the z of the neighbouring tiles' rim nodes -- disappears as
// well: a tile keeps r and P of its halo nodes and receives their q (published
// BEFORE the all-reduce and collected by the wave that does not sweep, while
// the sweep runs), so it forms the halo's z and d itself, bit-identical with
// the owner's.
//
// DIRECT (one-exchange solver only): the all-reduce gathers in one hop, for
// grids of 2 .. RES_DIRECT_GROUPS groups of RES_GROUP tiles (cg_exchange.h,
// "the direct gather").  It is compiled into instantiations of its own,
// which the host launches on such grids only (resident_enqueue): the pairs in flight per sweeping lane cost
// registers in a kernel that has none to spare, and with both forms in one
// kernel the register allocation of EVERY grid's iteration moved (three more
// spill reloads in the loop, 0.5 - 0.8 us per iteration at 16, 75 and 256
// tiles: profiles/cg_direct_gather.txt).
template <bool FUSED, bool ONE, bool TRACE, bool DIRECT = false>
__global__ void __launch_bounds__(RES_THREADS, 2)
cg_resident_kernel(ResArgs A)
{
    // (the stamps of tools/cg_trace.py cost registers in a kernel that has none
    // to spare: they are compiled into instantiations of their own)
    bool const tracing = TRACE && A.trace != nullptr;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    // launch-ahead Newton loop: the loop ended (or a solve gave up) while this
    // launch was already enqueued -- every workgroup reads the same words
    if (A.pipelined && (A.status[I_STOP] | A.status[I_STEP_ABORT]) != 0)
        return;
    int const tw = A.tw, th = A.th;
    int const LW = tw + 2, LH = th + 2;
    int const tile_nodes = tw * th;
    ResLds const L = resident_lds_layout(tw, th, ONE);
    double *dtile = lds + L.dtile;                        // [LH*LW][4]
    double *yl = lds + L.yl;                              // [tile_nodes][4]
    double *Pl = lds + L.Pl;                              // [4 | 3][tile_nodes][4]
    double *rl = lds + L.rl;                              // [tile_nodes][4] (ONE)
    double *fb = lds + L.fb;                              // [3*tw + 3*th][16]
    double *xl = lds + L.xl;                              // [tile_nodes][4]
    double *bl = lds + L.bl;                              // [tile_nodes][4] (!ONE)
    double *rh = lds + L.rh;                              // [ring][4] (ONE)
    double *Ph = lds + L.Ph;                              // [ring][16] (ONE)
    double *qhl = lds + L.qh;                             // [ring][4] (ONE)
    int *hnode = reinterpret_cast<int *>(lds + L.hinfo);  // [ring] (ONE)
    double *red = lds + L.red;
    int *flag = reinterpret_cast<int *>(red + RES_KINDS * RES_WAVES + RES_KINDS);

    int const tid = threadIdx.x;
    int const nblocks = (int)gridDim.x;
    int const tile = (int)blockIdx.x;
    int const tiles_y = (A.rows + th - 1) / th;
    int const ty = tile / A.tiles_x;
    int const tx = tile - ty * A.tiles_x;
    auto tile_exists = [&](int x, int y) {
        return x >= 0 && x < A.tiles_x && y >= 0 && y < tiles_y;
    };
    int const lx = tid % tw, ly = tid / tw;
    int const gx = tx * tw + lx, gy = ty * th + ly;
    bool const mine = tid < tile_nodes && gx < A.stride && gy < A.rows;
    int const n = mine ? gy * A.stride + gx : 0;
    int const lcore = (ly + 1) * LW + lx + 1;
    int const li = ly * tw + lx;             // index in the tile
    TileGeom const G = { tw, th, LW, lx, ly, li, lcore };
    // the exchanged vector of a rim node is read by the neighbouring tiles
    // (a grid of one tile has no neighbours: nothing is published)
    // ---- the compacted solve (fused one-exchange kernel) ----
    // The reference's system holds the active nodes only
    // (gauss_newton_step.cc:73-79, 91-105).  Here the rows of an inactive node
    // are zero, and so are its r, z, d, q and its terms of every sum -- exactly:
    //   * an inactive rim node publishes nothing and nobody polls for it (the
    //     neighbour takes q = 0, what the owner would have sent);
    //   * a tile without an active node says so in `ex->live` and LEAVES before
    //     it assembles anything: its CU is free, the all-reduce neither waits for
    //     it nor reads its slots (the first live member of a group sums it).
    // Both leave every total, every iterate and the iteration count bit-identical
    // (SMVS_CG_COMPACT=0 runs the full grid; tests/test_gpu_parity.py compares).
    bool compact = FUSED && ONE && !TRACE && nblocks > 1 && A.compact != 0;
    unsigned long long *livemap = reinterpret_cast<unsigned long long *>(lds + L.live);
    unsigned const live_tag = (unsigned)A.solve_tag;
    // every thread of the first RES_MAX_BLOCKS polls one tile's word; false after
    // a bounded wait.  On return the map is in LDS.
    auto gather_live_map = [&]() -> bool {
        bool ok = true;
        if (tid < RES_MAX_BLOCKS) {
            bool const need = tid < nblocks;
            unsigned w = 0u;
            for (unsigned spins = 0; need; ++spins) {
                w = __hip_atomic_load(&A.ex->live[tid], __ATOMIC_RELAXED,
                    __HIP_MEMORY_SCOPE_AGENT);
                if ((w & 0xFFFF0000u) == live_tag && (w & 3u) != 0u)
                    break;
                if (spins > (1u << 18)) {
                    __hip_atomic_store(&A.ex->timeout, 1u, __ATOMIC_RELAXED,
                        __HIP_MEMORY_SCOPE_AGENT);
                    ok = false;
                    w = 0u;
                    break;
                }
                __builtin_amdgcn_s_sleep(2);
            }
            unsigned long long const m = __ballot(need && (w & 1u) != 0u);
            if ((tid & 63) == 0)
                livemap[tid >> 6] = m;
        }
        // (workgroup-wide AND through the flag words of the all-reduce, which
        // are free outside an exchange -- __syncthreads_and would bring static
        // LDS into a kernel whose dynamic LDS is sized to the CU's 160 KB)
        bool const wave_ok = __all(ok);
        if ((tid & 63) == 0)
            flag[tid >> 6] = wave_ok ? 1 : 0;
        lds_barrier();
        bool all_ok = true;
#pragma unroll
        for (int wv = 0; wv < RES_WAVES; ++wv)
            all_ok = all_ok && flag[wv] != 0;
        lds_barrier();
        return all_ok;
    };
    auto tile_live = [&](int t) {
        return ((livemap[t >> 6] >> (t & 63)) & 1ull) != 0ull;
    };
    bool node_on = true;        // FUSED: the thread's node is active
    if (compact) {
        node_on = mine && A.active[n] != 0;
        bool const wave_any = __any(node_on);
        if ((tid & 63) == 0)
            flag[tid >> 6] = wave_any ? 1 : 0;
        lds_barrier();
        bool any = false;
#pragma unroll
        for (int wv = 0; wv < RES_WAVES; ++wv)
            any = any || flag[wv] != 0;
        lds_barrier();
        if (tid == 0)
            __hip_atomic_store(&A.ex->live[tile], live_tag | (any ? 1u : 2u), __ATOMIC_RELAXED,
                __HIP_MEMORY_SCOPE_AGENT);
        if (!any) {
            // what the prologue and the end of the solve do for the tile's nodes:
            // clear the flags of the step's node update, delta = 0, b = -g
            if (mine) {
                A.active_next[n] = 0;
                *reinterpret_cast<double4_r *>(A.x + (size_t)n * 4)
                    = (double4_r){ 0.0, 0.0, 0.0, 0.0 };
                *reinterpret_cast<double4_r *>(A.b + (size_t)n * 4)
                    = (double4_r){ -0.0, -0.0, -0.0, -0.0 };
            }
            if (tile == 0 && tid == 0) {
                A.status[I_ACTIVE_PATCHES] = A.status[I_LIVE_PATCHES];
                A.status[I_NUM_ACTIVE] = 0;
                A.scalars[S_SUMDIFF] = 0.0;
                A.scalars[S_COUNT_DIFF] = 0.0;
            }
            bool const got = gather_live_map();
            bool any_live = false;
            for (int w = 0; w < RES_MAX_BLOCKS / 64; ++w)
                any_live = any_live || livemap[w] != 0ull;
            if (!got || any_live)
                return;
            // no tile has an active node: a system of zeros, which the full grid
            // runs the way it always has (every workgroup is here and stays)
            compact = false;
            node_on = true;
        }
    }
    bool const rim = nblocks > 1 && mine && (!compact || node_on)
        && (lx == 0 || lx == tw - 1 || ly == 0 || ly == th - 1);
    size_t const N = (size_t)A.num_nodes;

    // halo ring position served by this thread
    int const ring = 2 * LW + 2 * th;
    bool const has_halo = tid < ring;
    int hx = 0, hy = 0;
    if (tid < LW) {
        hx = tid; hy = 0;
    } else if (tid < 2 * LW) {
        hx = tid - LW; hy = LH - 1;
    } else if (tid < 2 * LW + th) {
        hx = 0; hy = tid - 2 * LW + 1;
    } else if (has_halo) {
        hx = LW - 1; hy = tid - 2 * LW - th + 1;
    }
    int halo_node = -1, halo_ix = 0, halo_iy = 0;
    if (has_halo && tile_exists(tx, ty)) {
        halo_ix = tx * tw + hx - 1;
        halo_iy = ty * th + hy - 1;
        if (halo_ix >= 0 && halo_ix < A.stride && halo_iy >= 0 && halo_iy < A.rows)
            halo_node = halo_iy * A.stride + halo_ix;
    }
    int const lhalo = hy * LW + hx;
    if (tracing && blockIdx.x == 0 && tid == 0)
        A.trace[0] = (long long)wall_clock64();
    if (tracing && tid == 0)
        A.trace[TRACE_BLOCK_BASE + 4 * blockIdx.x + 0] = (long long)wall_clock64();
    // tag of the exchanged vectors: the solve id and the iteration that reads them
    unsigned const ztag = (unsigned)A.solve_tag;
    // block-Jacobi preconditioner (block_sparse_matrix.h:300-316): the
    // inverted diagonal block, kept un-inverted on NaN / zero pivot (Q12)
    auto invert_diagonal = [](double const (&d10)[10], double (&Pfull)[16]) {
        double const full[16] = { d10[0], d10[1], d10[2], d10[3],
            d10[1], d10[4], d10[5], d10[6], d10[2], d10[5], d10[7], d10[8],
            d10[3], d10[6], d10[8], d10[9] };
#pragma unroll
        for (int i = 0; i < 16; ++i)
            Pfull[i] = full[i];
        ldl_inverse4(Pfull);
        bool nancheck = false;
#pragma unroll
        for (int i = 0; i < 16; ++i)
            nancheck |= isnan(Pfull[i]);
#pragma unroll
        for (int i = 0; i < 16; ++i)
            Pfull[i] = nancheck ? full[i] : Pfull[i];
    };
    // ---- the matrix: five stored blocks in registers, the rim in LDS ----
    // (the diagonal block is symmetric, Q4: its upper triangle, 10 doubles)
    double hd[10];
    double hu[4][16];
    double gnode[4];          // gradient of the node
    double r[4], z[4];
    double v0[2] = { 0.0, 0.0 };   // z.r and g.g of this thread's node
    // x = 0, r = b = -g, z = P r of the thread's node (conjugate_gradient.h:86-118)
    // from hd / gnode; P goes to LDS
    auto init_own = [&]() {
        if (mine) {
            double const gg[4] = { gnode[0], gnode[1], gnode[2], gnode[3] };
            double Pfull[16];
            if (FUSED) {
                invert_diagonal(hd, Pfull);
            } else {
                const double4_r *P = reinterpret_cast<const double4_r *>(
                    A.Pinv + (size_t)n * 16);
#pragma unroll
                for (int row = 0; row < 4; ++row) {
                    double4_r const p = P[row];
                    Pfull[row * 4 + 0] = p.x; Pfull[row * 4 + 1] = p.y;
                    Pfull[row * 4 + 2] = p.z; Pfull[row * 4 + 3] = p.w;
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                r[k] = -gg[k];
            if (ONE) {
                double4_r *Pu = reinterpret_cast<double4_r *>(Pl);
                Pu[li] = (double4_r){ Pfull[0], Pfull[1], Pfull[2], Pfull[3] };
                Pu[tile_nodes + li] = (double4_r){ Pfull[5], Pfull[6], Pfull[7], Pfull[10] };
                Pu[2 * tile_nodes + li] = (double4_r){ Pfull[11], Pfull[15], 0.0, 0.0 };
                *reinterpret_cast<double4_r *>(rl + (size_t)li * 4)
                    = (double4_r){ r[0], r[1], r[2], r[3] };
            } else {
#pragma unroll
                for (int row = 0; row < 4; ++row)
                    *reinterpret_cast<double4_r *>(Pl + ((size_t)row * tile_nodes + li) * 4)
                        = (double4_r){ Pfull[row * 4 + 0], Pfull[row * 4 + 1],
                            Pfull[row * 4 + 2], Pfull[row * 4 + 3] };
            }
            precondition(Pfull, r, z);
            *reinterpret_cast<double4_r *>(xl + (size_t)li * 4)
                = (double4_r){ 0.0, 0.0, 0.0, 0.0 };
            if (ONE) {
                // b goes to HBM now (it is not needed again); d_1 = z_0
                *reinterpret_cast<double4_r *>(A.b + (size_t)n * 4)
                    = (double4_r){ r[0], r[1], r[2], r[3] };
                reinterpret_cast<double4_r *>(dtile)[lcore]
                    = (double4_r){ z[0], z[1], z[2], z[3] };
                *reinterpret_cast<double4_r *>(yl + (size_t)li * 4)
                    = (double4_r){ 0.0, 0.0, 0.0, 0.0 };
            } else {
                *reinterpret_cast<double4_r *>(bl + (size_t)li * 4)
                    = (double4_r){ r[0], r[1], r[2], r[3] };
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!ONE && rim)
                    st_granules(A.zg + ((size_t)n * 4 + k) * 2, ztag + 1u, z[k]);
                v0[0] += z[k] * r[k];
                v0[1] += gg[k] * gg[k];
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                r[k] = z[k] = 0.0;
        }
    };
    if constexpr (ONE) {
        // Order of the one-exchange prologue: halo, own diagonal block and P,
        // then the upper blocks -- the LDL^T inverses run before the 128
        // registers of the upper blocks are occupied.
        for (int i = tid; i < LH * LW * 4; i += RES_THREADS)
            dtile[i] = 0.0;   // (out-of-grid halo stays zero for the whole solve)
        // (LDS is not cleared between launches: a word a previous kernel left
        // where the exchange keeps its tags must not look like one of this
        // solve's -- tags are never 0)
        if (tid < RES_KINDS)
            group_mailbox(red).tag[tid] = 0u;
        if (tid < RES_WAVES)
            partial_tags(red).tag[tid] = 0u;
        lds_barrier();
        if (has_halo) {
            // (compacted: nobody publishes an inactive node's q -- it is zero)
            hnode[tid] = halo_node >= 0 && compact && A.active[halo_node] == 0 ? -1 : halo_node;
            // r and P of the halo node, with the operations of its owner
            double Ph16[16], gh[4] = { 0.0, 0.0, 0.0, 0.0 };
#pragma unroll
            for (int i = 0; i < 16; ++i)
                Ph16[i] = 0.0;
            if (halo_node >= 0) {
                if (FUSED) {
                    double hdh[10];
                    assemble_diagonal(A, halo_ix, halo_iy, hdh, gh);
                    invert_diagonal(hdh, Ph16);
                } else {
                    const double4_r *P = reinterpret_cast<const double4_r *>(
                        A.Pinv + (size_t)halo_node * 16);
#pragma unroll
                    for (int row = 0; row < 4; ++row) {
                        double4_r const p = P[row];
                        Ph16[row * 4 + 0] = p.x; Ph16[row * 4 + 1] = p.y;
                        Ph16[row * 4 + 2] = p.z; Ph16[row * 4 + 3] = p.w;
                    }
                    double4_r const gv = *reinterpret_cast<const double4_r *>(
                        A.g + (size_t)halo_node * 4);
                    gh[0] = gv.x; gh[1] = gv.y; gh[2] = gv.z; gh[3] = gv.w;
                }
            }
            double rhv[4], zh[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                rhv[k] = -gh[k];
            precondition(Ph16, rhv, zh);
            *reinterpret_cast<double4_r *>(rh + (size_t)tid * 4)
                = (double4_r){ rhv[0], rhv[1], rhv[2], rhv[3] };
#pragma unroll
            for (int row = 0; row < 4; ++row)
                *reinterpret_cast<double4_r *>(Ph + (size_t)tid * 16 + row * 4)
                    = (double4_r){ Ph16[row * 4 + 0], Ph16[row * 4 + 1],
                        Ph16[row * 4 + 2], Ph16[row * 4 + 3] };
            if (halo_node >= 0)
                reinterpret_cast<double4_r *>(dtile)[lhalo]
                    = (double4_r){ zh[0], zh[1], zh[2], zh[3] };
        }
        if (FUSED) {
            if (mine) {
                assemble_diagonal(A, gx, gy, hd, gnode);
                A.active_next[n] = 0;
            } else {
#pragma unroll
                for (int i = 0; i < 10; ++i)
                    hd[i] = 0.0;
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    gnode[i] = 0.0;
            }
            if (blockIdx.x == 0 && tid == 0) {
                A.status[I_ACTIVE_PATCHES] = A.status[I_LIVE_PATCHES];
                A.status[I_NUM_ACTIVE] = 0;
                A.scalars[S_SUMDIFF] = 0.0;
                A.scalars[S_COUNT_DIFF] = 0.0;
            }
        } else {
            const double4_r *src = reinterpret_cast<const double4_r *>(
                A.H9 + (size_t)n * 16);
            double4_r const zero4 = { 0, 0, 0, 0 };
            double4_r const r0 = mine ? src[0] : zero4, r1 = mine ? src[1] : zero4,
                r2 = mine ? src[2] : zero4, r3 = mine ? src[3] : zero4;
            hd[0] = r0.x; hd[1] = r0.y; hd[2] = r0.z; hd[3] = r0.w;
            hd[4] = r1.y; hd[5] = r1.z; hd[6] = r1.w;
            hd[7] = r2.z; hd[8] = r2.w;
            hd[9] = r3.w;
            double4_r const gv = mine ? *reinterpret_cast<const double4_r *>(
                A.g + (size_t)n * 4) : zero4;
            gnode[0] = gv.x; gnode[1] = gv.y; gnode[2] = gv.z; gnode[3] = gv.w;
        }
        init_own();
        if (FUSED) {
            assemble_upper(A, gx, gy, mine, hu);
        } else {
#pragma unroll
            for (int s = 1; s < 5; ++s) {
                const double4_r *src = reinterpret_cast<const double4_r *>(
                    A.H9 + ((size_t)s * N + (size_t)n) * 16);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    double4_r const v = mine ? src[q] : (double4_r){ 0, 0, 0, 0 };
                    hu[s - 1][4 * q + 0] = v.x; hu[s - 1][4 * q + 1] = v.y;
                    hu[s - 1][4 * q + 2] = v.z; hu[s - 1][4 * q + 3] = v.w;
                }
            }
        }
    } else if (FUSED) {
        // assembled here from the per-patch systems: H, g and P never go to
        // HBM.  Also what the assembly kernel does for the step's node update.
        NodeSystem S;
        assemble_node(A, gx, gy, mine, S);
#pragma unroll
        for (int i = 0; i < 10; ++i)
            hd[i] = S.hd[i];
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int i = 0; i < 16; ++i)
                hu[k][i] = S.hu[k][i];
#pragma unroll
        for (int i = 0; i < 4; ++i)
            gnode[i] = S.g[i];
        if (mine)
            A.active_next[n] = 0;
        if (blockIdx.x == 0 && tid == 0) {
            A.status[I_ACTIVE_PATCHES] = A.status[I_LIVE_PATCHES];
            A.status[I_NUM_ACTIVE] = 0;
            A.scalars[S_SUMDIFF] = 0.0;
            A.scalars[S_COUNT_DIFF] = 0.0;
        }
    } else {
        {
            const double4_r *src = reinterpret_cast<const double4_r *>(
                A.H9 + (size_t)n * 16);
            double4_r const zero4 = { 0, 0, 0, 0 };
            double4_r const r0 = mine ? src[0] : zero4, r1 = mine ? src[1] : zero4,
                r2 = mine ? src[2] : zero4, r3 = mine ? src[3] : zero4;
            hd[0] = r0.x; hd[1] = r0.y; hd[2] = r0.z; hd[3] = r0.w;
            hd[4] = r1.y; hd[5] = r1.z; hd[6] = r1.w;
            hd[7] = r2.z; hd[8] = r2.w;
            hd[9] = r3.w;
        }
#pragma unroll
        for (int s = 1; s < 5; ++s) {
            const double4_r *src = reinterpret_cast<const double4_r *>(
                A.H9 + ((size_t)s * N + (size_t)n) * 16);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                double4_r const v = mine ? src[q] : (double4_r){ 0, 0, 0, 0 };
                hu[s - 1][4 * q + 0] = v.x; hu[s - 1][4 * q + 1] = v.y;
                hu[s - 1][4 * q + 2] = v.z; hu[s - 1][4 * q + 3] = v.w;
            }
        }
        double4_r const gv = mine ? *reinterpret_cast<const double4_r *>(
            A.g + (size_t)n * 4) : (double4_r){ 0, 0, 0, 0 };
        gnode[0] = gv.x; gnode[1] = gv.y; gnode[2] = gv.z; gnode[3] = gv.w;
    }
    if (tracing && blockIdx.x == 0 && tid == 0)
        A.trace[2] = (long long)wall_clock64();   // own blocks in registers
    if (tracing && tid == 0)
        A.trace[TRACE_BLOCK_BASE + 4 * blockIdx.x + 1] = (long long)wall_clock64();
    // `low` holds two bits per lower slot s = 0..3 <-> (dx, dy) = (-1,-1),
    // (0,-1), (1,-1), (-1,0): 0 neighbour outside the grid, 1 neighbour inside
    // the tile (its contribution arrives through `yl`), 2 the neighbour's
    // block sits in the rim; `up` one bit per upper slot: the neighbour's row
    // lives in this tile.
    unsigned low = 0u, up = 0u;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        int const dx = s == 3 ? -1 : s - 1, dy = s == 3 ? 0 : -1;
        int const nx = gx + dx, ny = gy + dy;
        if (mine && nx >= 0 && nx < A.stride && ny >= 0) {
            int const mlx = lx + dx, mly = ly + dy;
            bool const in_tile = mly >= 0 && mlx >= 0 && mlx < tw;
            low |= (in_tile ? 1u : 2u) << (2 * s);
            if (!in_tile) {
                // block (row m, col n) is stored at m under its upper slot 8 - s
                double *dst = fb + (size_t)G.rim_index(s) * 16;
                if (FUSED) {
                    // (assembled below, one thread per rim block)
                } else {
                    int const m = ny * A.stride + nx;
                    const double4_r *src = reinterpret_cast<const double4_r *>(
                        A.H9 + ((size_t)(8 - s - 4) * N + (size_t)m) * 16);
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        reinterpret_cast<double4_r *>(dst)[e] = src[e];
                }
            }
        }
    }
    if (FUSED) {
        // The rim blocks, one thread each (with the tile node's own thread
        // doing up to three of them one after the other this phase was a
        // chain of ~8 memory latencies for a handful of threads).  The index
        // decodes as rim_index encodes: top row, left column (two slots),
        // right column.
        for (int r = tid; r < 3 * tw + 3 * th; r += RES_THREADS) {
            int rs, rlx, rly;
            if (r < 3 * tw) {
                rs = r / tw; rlx = r - rs * tw; rly = 0;
            } else if (r < 3 * tw + th) {
                rs = 0; rlx = 0; rly = r - 3 * tw;
            } else if (r < 3 * tw + 2 * th) {
                rs = 3; rlx = 0; rly = r - 3 * tw - th;
            } else {
                rs = 2; rlx = tw - 1; rly = r - 3 * tw - 2 * th;
            }
            int const dx = rs == 3 ? -1 : rs - 1, dy = rs == 3 ? 0 : -1;
            int const ngx = tx * tw + rlx, ngy = ty * th + rly;   // the tile node
            int const nx = ngx + dx, ny = ngy + dy;               // the row node
            bool const tile_node = ngx < A.stride && ngy < A.rows;
            bool const in_tile = rly + dy >= 0 && rlx + dx >= 0 && rlx + dx < tw;
            // (the column entries with rly = 0 belong to the top row's indices)
            bool const dup = r >= 3 * tw && r != 3 * tw + th && rly == 0;
            if (tile_node && !in_tile && !dup && nx >= 0 && nx < A.stride && ny >= 0)
                assemble_rim_block(A, nx, ny, rs, fb + (size_t)r * 16);
        }
    }
    if (tracing && blockIdx.x == 0 && tid == 0)
        A.trace[3] = (long long)wall_clock64();   // rim blocks in LDS
    if (tracing && tid == 0)
        A.trace[TRACE_BLOCK_BASE + 4 * blockIdx.x + 2] = (long long)wall_clock64();
    // upper slots 5..8 <-> (dx, dy) = (1,0), (-1,1), (0,1), (1,1)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int const s = 5 + k;
        int const dx = s % 3 - 1, dy = s / 3 - 1;
        int const mlx = lx + dx, mly = ly + dy;
        bool const in_tile = mine && mlx >= 0 && mlx < tw && mly < th
            && gx + dx < A.stride && gy + dy < A.rows;
        up |= (in_tile ? 1u : 0u) << k;
    }
    unsigned epoch = 1;
    bool alive = true;
    int reporter = 0;       // the workgroup that writes the result (compacted: the first live one)
    bool report_all = false;
    CgState st;
    if constexpr (!ONE) {
        // zero the direction tile (out-of-grid halo stays zero for the whole solve)
        for (int i = tid; i < LH * LW * 4; i += RES_THREADS)
            dtile[i] = 0.0;
        init_own();
    }
    if (tracing && blockIdx.x == 0 && tid == 0)
        A.trace[4] = (long long)wall_clock64();   // P, r, z done
    if (tracing && tid == 0)
        A.trace[TRACE_BLOCK_BASE + 4 * blockIdx.x + 3] = (long long)wall_clock64();
    st.q0 = -0.0;
    st.iter = 1;
    st.done = 0;
    st.info = SMVS_CG_MAX_ITERATIONS;
    st.pad = 0;
    st.rr = st.tol = st.gnorm = 0.0;

    auto stamp = [&](int k, int point) {
        if (tracing && (int)blockIdx.x == A.trace_wg && tid == 0 && k <= TRACE_ITERS)
            A.trace[k * TRACE_POINTS + point] = (long long)wall_clock64();
    };
    if constexpr (!ONE) {
        alive = grid_allreduce<2, 3>(A.ex, ztag, epoch++, nblocks, v0, red, flag,
            NoIdleWork());
        st.rr = v0[0];
        st.gnorm = sqrt(v0[1]);
        st.tol = A.fixed_tolerance < 0.0 ? st.gnorm * 0.01 : A.fixed_tolerance;
        stamp(0, 1);
        // ---- iterations (conjugate_gradient.h:123-198) ----
        double beta = 0.0;
        for (int k = 1; alive && k < A.max_iterations; ++k) {
            stamp(k, 0);
            // d_k = z + beta d_{k-1}: own node and halo, in LDS
            {
#pragma clang fp contract(off)
                double4_r *dt = reinterpret_cast<double4_r *>(dtile);
                if (mine) {
                    double4_r const old = dt[lcore];
                    dt[lcore] = (double4_r){ z[0] + beta * old.x, z[1] + beta * old.y,
                        z[2] + beta * old.z, z[3] + beta * old.w };
                    *reinterpret_cast<double4_r *>(yl + (size_t)li * 4)
                        = (double4_r){ 0.0, 0.0, 0.0, 0.0 };
                }
                if (halo_node >= 0) {
                    // the neighbour's z of the previous iteration: poll its eight
                    // granules until all carry this iteration's tag
                    double zh[4] = { 0.0, 0.0, 0.0, 0.0 };
                    (void)poll_node_granules(A.zg + (size_t)halo_node * 8,
                        ztag + (unsigned)k, A.ex, zh);
                    double4_r const old = dt[lhalo];
                    dt[lhalo] = (double4_r){ zh[0] + beta * old.x, zh[1] + beta * old.y,
                        zh[2] + beta * old.z, zh[3] + beta * old.w };
                }
            }
            lds_barrier();
            stamp(k, 1);
            double acc[4] = { 0.0, 0.0, 0.0, 0.0 };
            double dself[4];
            tile_product(G, dtile, yl, fb, hd, hu, low, up, mine, acc, dself);
            stamp(k, 2);
            double dad[1] = { 0.0 };
            if (mine)
                dad[0] = dself[0] * acc[0] + dself[1] * acc[1]
                    + dself[2] * acc[2] + dself[3] * acc[3];
            stamp(k, 3);
            if (!(alive = grid_allreduce<1, 3>(A.ex, ztag, epoch++, nblocks, dad, red,
                      flag, NoIdleWork())))
                break;
            stamp(k, 4);
            double const alpha = st.rr / dad[0];
            // x += alpha d, r -= alpha Ad, z = P r: x, b and P in LDS; only the rim
            // publishes its z (as granules: nothing to drain before the all-reduce)
            double v3[3] = { 0.0, 0.0, 0.0 };
            if (mine) {
#pragma clang fp contract(off)
                double4_r *xp = reinterpret_cast<double4_r *>(xl + (size_t)li * 4);
                double4_r const xv = *xp;
                double4_r const bv = *reinterpret_cast<const double4_r *>(
                    bl + (size_t)li * 4);
                double const xn[4] = { xv.x + alpha * dself[0], xv.y + alpha * dself[1],
                    xv.z + alpha * dself[2], xv.w + alpha * dself[3] };
                double const bo[4] = { bv.x, bv.y, bv.z, bv.w };
                *xp = (double4_r){ xn[0], xn[1], xn[2], xn[3] };
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    r[q] = r[q] - alpha * acc[q];
#pragma unroll
                for (int row = 0; row < 4; ++row) {
                    double4_r const p = *reinterpret_cast<const double4_r *>(
                        Pl + ((size_t)row * tile_nodes + li) * 4);
                    double zi = 0.0;
                    zi += p.x * r[0];
                    zi += p.y * r[1];
                    zi += p.z * r[2];
                    zi += p.w * r[3];
                    z[row] = zi;
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (rim)
                        st_granules(A.zg + ((size_t)n * 4 + q) * 2,
                            ztag + (unsigned)k + 1u, z[q]);
                    v3[0] += r[q] * r[q];
                    v3[1] += xn[q] * (bo[q] + r[q]);
                    v3[2] += z[q] * r[q];
                }
            }
            stamp(k, 5);
            if (!(alive = grid_allreduce<3, 3>(A.ex, ztag, epoch++, nblocks, v3, red,
                      flag, NoIdleWork())))
                break;
            stamp(k, 6);
            // termination tests of iteration k (conjugate_gradient.h:136-198)
            double const new_rr = v3[0];
            double const Q1 = -1.0 * v3[1];
            int done = 0, info = SMVS_CG_MAX_ITERATIONS, iter_out = k + 1;
            if (new_rr < st.tol) {
                done = 1; info = SMVS_CG_CONVERGENCE; iter_out = k;
            } else {
                double const zeta = k * (Q1 - st.q0) / Q1;
                if (zeta < A.q_tolerance) {
                    done = 1; info = SMVS_CG_CONVERGENCE; iter_out = k;
                } else if (k + 1 >= A.max_iterations) {
                    done = 1;
                }
            }
            beta = v3[2] / st.rr;
            st.rr = v3[2];
            st.q0 = Q1;
            st.iter = iter_out;
            st.done = done;
            st.info = info;
            if (done)
                break;
        }
    } else {
        // ---- one exchange per iteration ----
        lds_barrier();          // d_1 (own and halo) in the tile
        stamp(0, 1);
        // who takes part in the exchanges: everybody, or (compacted) the tiles
        // with an active node -- their words have been out since they started
        LiveSet live;
        int const ngroups_all = (nblocks + RES_GROUP - 1) / RES_GROUP;
        live.leads = ngroups_all > 1 && tile % RES_GROUP == 0;
        live.bits = DIRECT ? 3u | (((1u << RES_DIRECT_GROUPS) - 1u) << 2) : 3u;
        if (compact) {
            // (a map that did not arrive: the solve is given up, and since nobody
            // knows who the first live tile is, every workgroup says so)
            if (!gather_live_map())
                alive = false, report_all = true;
            int const member0 = tile - tile % RES_GROUP, j = tid & 15;
            auto group_live = [&](int g) {
                return ((livemap[(g * RES_GROUP) >> 6] >> ((g * RES_GROUP) & 63)) & 0xFFFFull)
                    != 0ull;
            };
            unsigned const mine16 = (unsigned)((livemap[member0 >> 6] >> (member0 & 63))
                & 0xFFFFull);
            live.leads = ngroups_all > 1 && mine16 != 0u
                && (int)__builtin_ctz(mine16) == tile - member0;
            live.bits = (member0 + j < nblocks && tile_live(member0 + j) ? 1u : 0u)
                | (j < ngroups_all && group_live(j) ? 2u : 0u);
            // (the direct gather: member j of each group)
            if constexpr (DIRECT) {
#pragma unroll
                for (int g = 0; g < RES_DIRECT_GROUPS; ++g)
                    if (RES_GROUP * g + j < nblocks && tile_live(RES_GROUP * g + j))
                        live.bits |= 4u << g;
            }
            // the first live tile reports the result
            reporter = 0;
            for (int w = RES_MAX_BLOCKS / 64 - 1; w >= 0; --w)
                if (livemap[w] != 0ull)
                    reporter = 64 * w + (int)__builtin_ctzll(livemap[w]);
        }
        double xbr = 0.0;       // x.(b + r) of the current vectors
        double zr_part = 0.0;   // this node's z.r, formed where z is (end of the last iteration)
        __amdgpu_buffer_rsrc_t const zbuf = pair_buffer(A.zg, (size_t)A.num_nodes * 128);
        // byte offset of a node's four pairs in `zg`: by node id
        auto zg_at = [&](unsigned par, unsigned node) {
            return ((par * (unsigned)A.num_nodes + node) * 4u) * 16u;
        };
        auto skew = [&](int k, int point, int who) {
            if (tracing && k == TRACE_SKEW_ITER && tid == who)
                A.trace[TRACE_SKEW_BASE + 4 * blockIdx.x + point] = (long long)wall_clock64();
        };
        for (int k = 1; alive && k < A.max_iterations; ++k) {
            stamp(k, 0);
            skew(k, 0, 0);
            auto sweep_mark = [&](int point, long long value) {
                if (point >= 16) {
                    // per-wave stamps of one iteration
                    if (tracing && (int)blockIdx.x == A.trace_wg
                        && (tid & 63) == 0 && k == TRACE_SKEW_ITER)
                        A.trace[TRACE_WAVE_BASE + 8 * (tid >> 6) + point - 16]
                            = (long long)wall_clock64();
                    return;
                }
                if (tracing && (int)blockIdx.x == A.trace_wg && tid == 64
                    && k <= TRACE_ITERS)
                    A.trace[k * TRACE_POINTS + point] = value >= 0 ? value
                        : (long long)wall_clock64();
            };
            sweep_mark(16, -1);
            double acc[4] = { 0.0, 0.0, 0.0, 0.0 };   // q = H d
            double dself[4];
            tile_product(G, dtile, yl, fb, hd, hu, low, up, mine, acc, dself);
            stamp(k, 1);
            sweep_mark(17, -1);
            // the sums (z.q + w.r is taken as 2 w.r: P is symmetric, z.q = r.(P q))
            double v8[8] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
            // The rim's q for the neighbouring tiles' halo.
            unsigned const hpar = (unsigned)k & 1u;
            auto publish_rim = [&]() {
                if (rim) {
                    unsigned const t = ztag + (unsigned)k;
                    unsigned const at = zg_at(hpar, (unsigned)n);
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        st_pair16(zbuf, at + (unsigned)q * 16u, t, acc[q]);
                }
            };
            // (as soon as q is known, in front of the sums although the exchange
            // waits for those: the write-through stores of a CU drain slowly,
            // ~380 of them in 3-5 us, and issuing them takes a wave up to 1 us --
            // behind the sums, the halo arrived 3 us later; here the issue
            // overlaps the arithmetic of the sums.  Also measured and dropped:
            // the rim staged in LDS and stored behind the sums by two waves as
            // whole 64-byte records, four lanes per node -- fewer, fuller
            // writes, but the halo arrives late: 9.9 instead of 9.1 us.)
            publish_rim();
            sweep_mark(19, -1);
            if (mine) {
#pragma clang fp contract(off)
                double Pn[4][4];
                load_symmetric(Pl, tile_nodes, li, Pn);
                double4_r const rv = *reinterpret_cast<const double4_r *>(
                    rl + (size_t)li * 4);
                double const r[4] = { rv.x, rv.y, rv.z, rv.w };
#pragma unroll
                for (int row = 0; row < 4; ++row) {
                    double wi = 0.0;
                    wi += Pn[row][0] * acc[0];
                    wi += Pn[row][1] * acc[1];
                    wi += Pn[row][2] * acc[2];
                    wi += Pn[row][3] * acc[3];
                    v8[3] += 2.0 * (wi * r[row]);
                    v8[4] += wi * acc[row];
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    v8[0] += dself[q] * acc[q];
                    v8[1] += r[q] * acc[q];
                    v8[2] += acc[q] * acc[q];
                    v8[5] += dself[q] * r[q];
                    v8[6] += r[q] * r[q];
                }
                v8[7] = zr_part;
            }
            sweep_mark(18, -1);
            stamp(k, 2);
            skew(k, 1, 0);
            // The sweeping waves run the two-level all-reduce; wave 0 meanwhile
            // collects the q of the halo nodes into LDS.
            // (Measured and dropped: four adjacent lanes reading the four pairs of
            // one node, a quarter of the requests per poll round -- the extra
            // registers cost more than the requests: 174 instead of 176 M
            // patch-steps/s.)
            auto fetch_halo = [&]() {
                if (nblocks > 1)
                    nap(A.wait_halo);
                for (int hs = tid; hs < ring; hs += 64) {
                    int const node = hnode[hs];
                    double qv[4] = { 0.0, 0.0, 0.0, 0.0 };
                    if (node >= 0)
                        (void)poll_node_pairs(zbuf, zg_at(hpar, (unsigned)node),
                            ztag + (unsigned)k, A.ex, qv, A.wait_poll);
                    *reinterpret_cast<double4_r *>(qhl + (size_t)hs * 4)
                        = (double4_r){ qv[0], qv[1], qv[2], qv[3] };
                }
            };
            auto other_waves = [&](int wave) {
                if (wave == 0) {
                    fetch_halo();
                    stamp(k, 7);
                    skew(k, 3, 0);
                }
            };
            alive = grid_allreduce_tree<8, DIRECT>(A.ex, ztag, epoch++, nblocks, live, v8, red,
                flag, other_waves, sweep_mark, A.wait_member, A.wait_poll);
            if (!alive)
                break;
            stamp(k, 3);
            skew(k, 2, 0);
            sweep_mark(22, -1);      // per wave: the totals are in, the update starts
            double const dq = v8[0], rq = v8[1], qq = v8[2], s1 = v8[3], wq = v8[4],
                dr = v8[5], rr = v8[6];
            // z.r of the current vectors, summed directly like r.r (d_1 = z_0:
            // in the first iteration it is d.r); only the values one step ahead
            // come from the recurrences, so no rounding error is carried from
            // iteration to iteration
            double const zr = k == 1 ? dr : v8[7];
            if (k == 1) {
                // r_0 = -g
                st.gnorm = sqrt(rr);
                st.tol = A.fixed_tolerance < 0.0 ? st.gnorm * 0.01 : A.fixed_tolerance;
            }
            double const alpha = zr / dq;
            double const new_rr = __builtin_fma(alpha,
                __builtin_fma(alpha, qq, -2.0 * rq), rr);
            double const new_zr = __builtin_fma(alpha,
                __builtin_fma(alpha, wq, -s1), zr);
            double const new_xbr = __builtin_fma(alpha,
                __builtin_fma(-alpha, dq, 2.0 * dr), xbr);
            // termination tests of iteration k (conjugate_gradient.h:136-198)
            double const Q1 = -1.0 * new_xbr;
            int done = 0, info = SMVS_CG_MAX_ITERATIONS, iter_out = k + 1;
            if (new_rr < st.tol) {
                done = 1; info = SMVS_CG_CONVERGENCE; iter_out = k;
            } else {
                double const zeta = k * (Q1 - st.q0) / Q1;
                if (zeta < A.q_tolerance) {
                    done = 1; info = SMVS_CG_CONVERGENCE; iter_out = k;
                } else if (k + 1 >= A.max_iterations) {
                    done = 1;
                }
            }
            double const beta = new_zr / zr;
            // x += alpha d, r -= alpha q, z = P r, d = z + beta d: own node, and
            // r, z, d of the halo with the same operations
            {
#pragma clang fp contract(off)
                double4_r *dt = reinterpret_cast<double4_r *>(dtile);
                if (mine) {
                    double4_r *xp = reinterpret_cast<double4_r *>(xl + (size_t)li * 4);
                    double4_r const xv = *xp;
                    *xp = (double4_r){ xv.x + alpha * dself[0], xv.y + alpha * dself[1],
                        xv.z + alpha * dself[2], xv.w + alpha * dself[3] };
                    if (!done) {
                        double4_r *rp = reinterpret_cast<double4_r *>(rl + (size_t)li * 4);
                        double4_r const rv = *rp;
                        double const r[4] = { rv.x - alpha * acc[0], rv.y - alpha * acc[1],
                            rv.z - alpha * acc[2], rv.w - alpha * acc[3] };
                        *rp = (double4_r){ r[0], r[1], r[2], r[3] };
                        double Pn[4][4];
                        load_symmetric(Pl, tile_nodes, li, Pn);
                        double zn[4];
#pragma unroll
                        for (int row = 0; row < 4; ++row) {
                            double zi = 0.0;
                            zi += Pn[row][0] * r[0];
                            zi += Pn[row][1] * r[1];
                            zi += Pn[row][2] * r[2];
                            zi += Pn[row][3] * r[3];
                            zn[row] = zi;
                        }
                        {
                            double t = 0.0;
                            t += zn[0] * r[0];
                            t += zn[1] * r[1];
                            t += zn[2] * r[2];
                            t += zn[3] * r[3];
                            zr_part = t;
                        }
                        dt[lcore] = (double4_r){ zn[0] + beta * dself[0],
                            zn[1] + beta * dself[1], zn[2] + beta * dself[2],
                            zn[3] + beta * dself[3] };
                        *reinterpret_cast<double4_r *>(yl + (size_t)li * 4)
                            = (double4_r){ 0.0, 0.0, 0.0, 0.0 };
                    }
                }
                if (!done && halo_node >= 0) {
                    double4_r *rp = reinterpret_cast<double4_r *>(rh + (size_t)tid * 4);
                    double4_r const rv = *rp;
                    double4_r const qv = *reinterpret_cast<const double4_r *>(
                        qhl + (size_t)tid * 4);
                    double const rn[4] = { rv.x - alpha * qv.x, rv.y - alpha * qv.y,
                        rv.z - alpha * qv.z, rv.w - alpha * qv.w };
                    *rp = (double4_r){ rn[0], rn[1], rn[2], rn[3] };
                    double zh[4];
#pragma unroll
                    for (int row = 0; row < 4; ++row) {
                        double4_r const p = *reinterpret_cast<const double4_r *>(
                            Ph + (size_t)tid * 16 + row * 4);
                        double zi = 0.0;
                        zi += p.x * rn[0];
                        zi += p.y * rn[1];
                        zi += p.z * rn[2];
                        zi += p.w * rn[3];
                        zh[row] = zi;
                    }
                    double4_r const old = dt[lhalo];
                    dt[lhalo] = (double4_r){ zh[0] + beta * old.x, zh[1] + beta * old.y,
                        zh[2] + beta * old.z, zh[3] + beta * old.w };
                }
            }
            stamp(k, 4);
            sweep_mark(23, -1);      // per wave: own node (and, lanes < ring, halo node) updated
            xbr = new_xbr;
            st.rr = new_zr;
            st.q0 = Q1;
            st.iter = iter_out;
            st.done = done;
            st.info = info;
            if (done)
                break;
            lds_barrier();      // d_{k+1} in the tile
        }
    }

    // the solution (and b, which the streaming solver also leaves) go to HBM
    if (mine) {
        *reinterpret_cast<double4_r *>(A.x + (size_t)n * 4)
            = *reinterpret_cast<const double4_r *>(xl + (size_t)li * 4);
        if (!ONE)
            *reinterpret_cast<double4_r *>(A.b + (size_t)n * 4)
                = *reinterpret_cast<const double4_r *>(bl + (size_t)li * 4);
    }
    if ((tile == reporter || report_all) && tid == 0) {
        // (a halo wait of any workgroup that gave up raised the exchange's flag)
        bool const late_timeout = __hip_atomic_load(&A.ex->timeout, __ATOMIC_RELAXED,
            __HIP_MEMORY_SCOPE_AGENT) != 0u;
        int const failed = alive && !late_timeout && !(A.pipelined & RES_TEST_GIVE_UP) ? 0 : 1;
        if (!st.done && !failed) {
            // max_iterations <= 1 never reaches here (handled by the host)
            st.done = 1;
        }
        A.state[0] = st;
        A.status[I_DONE] = failed ? 0 : 1;
        A.status[I_INFO] = st.info;
        A.status[I_ITER] = st.iter;
        if (failed && A.pipelined)
            A.status[I_STEP_ABORT] = ABORT_SOLVER;   // the enqueued steps do nothing
        __hip_atomic_store(A.progress + PROGRESS_INFO, st.info, __ATOMIC_RELAXED,
            __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(A.progress + PROGRESS_ITERS, st.iter, __ATOMIC_RELAXED,
            __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(A.progress + PROGRESS_GAVE_UP, failed, __ATOMIC_RELAXED,
            __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(A.progress + PROGRESS_DONE, progress_done_word(A.solve_tag), __ATOMIC_RELEASE,
            __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

size_t
resident_lds_bytes(int tw, int th, bool one)
{
    return resident_lds_layout(tw, th, one).total * sizeof(double);
}

// The plan (cg_resident_plan.h) of the context's grid.
// (once per grid: a Newton step asks for the plan, a loop three more times)
static bool
resident_plan(const smvs_ctx *ctx, ResidentPlan *plan)
{
    smvs_ctx::ResidentPlanMemo &m = ctx->res_plan;
    if (m.stride != ctx->node_stride || m.nodes != ctx->num_nodes
        || m.solver_mode != (int)ctx->solver_mode || m.cus != ctx->resident_cus) {
        static int const ref_order_tiles = [] {
            const char *e = std::getenv("SMVS_REF_ORDER_TILES");
            int const n = e != nullptr ? std::atoi(e) : 1;
            return n < 0 ? 0 : n;
        }();
        ResidentPlan p = {};
        m.ok = compute_resident_plan(ctx->node_stride, ctx->num_nodes / ctx->node_stride,
            std::min(ctx->resident_cus, RES_MAX_BLOCKS), ctx->solver_mode,
            ref_order_tiles, &p);
        m.stride = ctx->node_stride;
        m.nodes = ctx->num_nodes;
        m.solver_mode = (int)ctx->solver_mode;
        m.cus = ctx->resident_cus;
        m.tw = p.tw; m.th = p.th; m.one = p.one ? 1 : 0; m.blocks = p.blocks;
    }
    plan->tw = m.tw; plan->th = m.th; plan->one = m.one != 0; plan->blocks = m.blocks;
    return m.ok;
}

// the context's device has that many CUs (0: HIP error)
static int
resident_cus(smvs_ctx *ctx)
{
    if (ctx->resident_cus == 0) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, physical_device(ctx->device)) != hipSuccess)
            return 0;
        ctx->resident_cus = prop.multiProcessorCount;
    }
    return ctx->resident_cus;
}

// Does the resident solver take this system?  (grid fits the chip's CUs and
// LDS, not disabled by SMVS_CG_RESIDENT=0 or by an earlier failure)
bool
cg_resident_applies(smvs_ctx *ctx, int max_iterations)
{
    if (ctx->resident_disabled || max_iterations <= 1 || !ctx->has_surface
        || ctx->solver_mode == SMVS_SOLVER_STREAMING)
        return false;
    // the exchange tags carry the epoch (<= 2 per iteration + 1) in their low
    // 16 bits beside the solve id: longer solves take the streaming kernels
    if (2 * max_iterations + 1 > 0xFFFF)
        return false;
    static int const env_off = [] {
        const char *e = std::getenv("SMVS_CG_RESIDENT");
        return e != nullptr && e[0] == '0' ? 1 : 0;
    }();
    if (env_off)
        return false;
    if (resident_cus(ctx) == 0)
        return false;
    ResidentPlan plan;
    if (!resident_plan(ctx, &plan))
        return false;
    if ((size_t)ctx->num_nodes * 5 * 16 >= (size_t)1 << 32)
        return false;
    return true;
}

static DeviceTileBudget g_resident_budget[16];

// The tile budget (tile_budget.h) of the GPU behind a logical device: logical
// devices mapped onto one GPU share its CUs.
DeviceTileBudget &
cg_resident_budget(int device)
{
    int const physical = physical_device(device);
    DeviceTileBudget &budget = g_resident_budget[physical & 15];
    if (!budget.is_bound()) {
        hipDeviceProp_t prop;
        int capacity = RES_MAX_BLOCKS;
        if (hipGetDeviceProperties(&prop, physical) == hipSuccess
            && prop.multiProcessorCount < capacity)
            capacity = prop.multiProcessorCount;
        // the same GPU may have different indices in different processes
        // (HIP_VISIBLE_DEVICES): name the file after the PCI bus id
        char bus[64] = "";
        if (hipDeviceGetPCIBusId(bus, (int)sizeof(bus), physical) != hipSuccess)
            std::snprintf(bus, sizeof(bus), "index%d", physical);
        budget.bind(capacity, bus);
    }
    return budget;
}

int
cg_resident_tiles(smvs_ctx *ctx)
{
    ResidentPlan plan;
    if (resident_cus(ctx) == 0 || !resident_plan(ctx, &plan))
        return 0;
    return plan.blocks;
}

// Launches the solver (the caller holds its tiles of the budget and has checked
// cg_resident_applies).  pipelined: the Newton loop's launch-ahead mode -- the
// kernel leaves at once when status[I_STOP] / [I_STEP_ABORT] is set, raises
// I_STEP_ABORT itself when it gives up, and nobody waits on the progress words.
// *solve_tag_out: the tag the progress words will carry.
static int
resident_enqueue(smvs_ctx *ctx, int max_iterations, double error_tolerance,
    double q_tolerance, bool fused, bool pipelined, long long *trace_dev,
    int *solve_tag_out, int *num_tiles_out, bool test_give_up = false)
{
    int const stride = ctx->node_stride;
    int const rows = ctx->num_nodes / stride;
    ResidentPlan plan;
    if (!resident_plan(ctx, &plan)) {
        set_error("resident_enqueue: the grid does not fit the resident solver");
        return SMVS_ERR_STATE;
    }
    int const tw = plan.tw, th = plan.th;
    int const tiles_x = (stride + tw - 1) / tw;
    int const num_tiles = plan.blocks;   // workgroups of the launch
    bool const one = plan.one;
    size_t const lds_bytes = resident_lds_bytes(tw, th, one);

    int rc;
    if (ctx->res_work == nullptr) {
        if ((rc = device_alloc(&ctx->res_work,
                 sizeof(ResExchange) / sizeof(double) + 8)) != SMVS_OK)
            return rc;
        SMVS_HIP_CHECK(hipMemsetAsync(ctx->res_work, 0, sizeof(ResExchange),
            ctx->stream));
    }
    // (the solver takes grids of at most RES_MAX_BLOCKS tiles of RES_THREADS nodes)
    size_t const zx_nodes = std::min(ctx->cap_nodes, (size_t)RES_MAX_BLOCKS * RES_THREADS);
    if (ctx->res_zx_cap < (size_t)ctx->num_nodes) {
        // [2][zx_nodes][4][2] words of `zg`
        if ((rc = device_alloc(&ctx->res_zx, zx_nodes * 16)) != SMVS_OK) {
            ctx->res_zx_cap = 0;
            return rc;
        }
        SMVS_HIP_CHECK(hipMemsetAsync(ctx->res_zx, 0, zx_nodes * 16 * sizeof(double),
            ctx->stream));
        ctx->res_zx_cap = zx_nodes;
    }
    {
        const void *kernels[7] = {
            reinterpret_cast<const void *>(cg_resident_kernel<false, true, false, true>),
            reinterpret_cast<const void *>(cg_resident_kernel<true, true, false, true>),
            reinterpret_cast<const void *>(cg_resident_kernel<false, false, false>),
            reinterpret_cast<const void *>(cg_resident_kernel<true, false, false>),
            reinterpret_cast<const void *>(cg_resident_kernel<false, true, false>),
            reinterpret_cast<const void *>(cg_resident_kernel<true, true, false>),
            reinterpret_cast<const void *>(cg_resident_kernel<true, true, true>) };
        for (const void *k : kernels)
            if ((rc = allow_dynamic_lds(ctx->device, k, lds_bytes)) != SMVS_OK)
                return rc;
    }

    ResArgs A;
    A.H9 = ctx->H9;
    A.Pinv = ctx->Pinv;
    A.g = ctx->g;
    A.x = ctx->x;
    A.b = ctx->b;
    A.zg = reinterpret_cast<unsigned long long *>(ctx->res_zx);
    A.ex = reinterpret_cast<ResExchange *>(ctx->res_work);
    A.state = reinterpret_cast<CgState *>(ctx->cg_state);
    A.status = ctx->status;
    A.progress = ctx->cg_progress;
    ctx->cg_solve_id = (ctx->cg_solve_id + 1) & 0x7FFF;
    if (ctx->cg_solve_id == 0) {
        // The 15-bit solve id starts over: a granule that no solve has
        // overwritten since the id was last used (a slot of an epoch only a
        // longer solve reaches) would carry a matching tag.  Clear both
        // exchange areas, once per 32,767 solves.
        ctx->cg_solve_id = 1;
        SMVS_HIP_CHECK(hipMemsetAsync(ctx->res_work, 0, sizeof(ResExchange),
            ctx->stream));
        SMVS_HIP_CHECK(hipMemsetAsync(ctx->res_zx, 0,
            ctx->res_zx_cap * 16 * sizeof(double), ctx->stream));
    }
    A.solve_tag = ctx->cg_solve_id << 16;
    A.num_nodes = ctx->num_nodes;
    A.stride = stride;
    A.rows = rows;
    A.tw = tw;
    A.th = th;
    A.tiles_x = tiles_x;
    A.num_tiles = num_tiles;
    A.max_iterations = max_iterations;
    A.q_tolerance = q_tolerance;
    A.fixed_tolerance = error_tolerance;
    A.Hp = ctx->Hp;
    A.gp = ctx->gp;
    A.layout = patch_layout(ctx);
    A.patch_valid = ctx->patch_valid;
    A.active = ctx->active;
    A.active_next = ctx->active_next;
    A.scalars = ctx->scalars;
    A.npx = ctx->npx;
    A.npy = ctx->npy;
    A.zeros = ctx->zero_block;
    {
        // polling cadence (the measured defaults; SMVS_CG_WAIT="halo,member,poll"
        // overrides them for experiments): the exchange gains 1.5 us per iteration
        // when the halo's polls start 1 us late (they compete with the
        // write-through stores of the rim)
        struct Knobs { int halo = -1, member = 3, poll = 0; };
        static Knobs const knobs = [] {
            Knobs k;
            if (const char *e = std::getenv("SMVS_CG_WAIT"))
                (void)std::sscanf(e, "%d,%d,%d", &k.halo, &k.member, &k.poll);
            return k;
        }();
        // (the full grid only: at 64 tiles the wait changes nothing, 6.95 against
        // 6.86 us per iteration, at 16 tiles it costs 0.5 us)
        A.wait_halo = knobs.halo >= 0 ? knobs.halo : num_tiles <= 64 ? 0 : 4;
        A.wait_member = knobs.member;
        A.wait_poll = knobs.poll;
    }
    {
        static int const compact = [] {
            const char *e = std::getenv("SMVS_CG_COMPACT");
            return e != nullptr && e[0] == '0' ? 0 : 1;
        }();
        A.compact = compact;
    }
    // which form the all-reduce of the one-exchange solver takes, by the number
    // of groups of RES_GROUP tiles alone: SMVS_CG_GATHER=tree (two levels
    // whenever there is more than one group), direct (one hop up to
    // RES_DIRECT_GROUPS groups) or the largest number of groups that gathers in
    // one hop.  The totals have the same bits either way.
    static int const direct_groups = [] {
        const char *e = std::getenv("SMVS_CG_GATHER");
        if (e == nullptr || e[0] == '\0')
            return RES_DIRECT_GROUPS_DEFAULT;
        if (std::strcmp(e, "tree") == 0)
            return 0;
        if (std::strcmp(e, "direct") == 0)
            return RES_DIRECT_GROUPS;
        return std::min(std::max(std::atoi(e), 0), RES_DIRECT_GROUPS);
    }();
    int const ngroups = (num_tiles + RES_GROUP - 1) / RES_GROUP;
    // (the stamps of tools/cg_trace.py exist in the two-level kernels only)
    bool const direct = one && trace_dev == nullptr && ngroups > 1 && ngroups <= direct_groups;
    A.trace = trace_dev;
    {
        static int const wg = [] {
            const char *e = std::getenv("SMVS_CG_TRACE_WG");
            return e != nullptr ? std::atoi(e) : 0;
        }();
        A.trace_wg = wg;
    }
    A.pipelined = pipelined ? RES_PIPELINED | (test_give_up ? RES_TEST_GIVE_UP : 0) : 0;
    *solve_tag_out = A.solve_tag;
    *num_tiles_out = num_tiles;
    {
        ScopedKernelTimer timer(ctx, SMVS_K_CG_RESIDENT);
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(num_tiles), dim3(RES_THREADS), lds_bytes,
                ctx->stream, A);
        };
        // (stamps: the fused one-exchange kernel only, what tools/cg_trace.py runs)
        if (direct && fused)
            launch(cg_resident_kernel<true, true, false, true>);
        else if (direct)
            launch(cg_resident_kernel<false, true, false, true>);
        else if (fused && one && trace_dev != nullptr)
            launch(cg_resident_kernel<true, true, true>);
        else if (fused && one)
            launch(cg_resident_kernel<true, true, false>);
        else if (fused)
            launch(cg_resident_kernel<true, false, false>);
        else if (one)
            launch(cg_resident_kernel<false, true, false>);
        else
            launch(cg_resident_kernel<false, false, false>);
    }
    SMVS_HIP_CHECK(hipGetLastError());
    return SMVS_OK;
}

// A resident solve gave up (the caller has waited for the kernel): its
// workgroups were not all resident.  Never try again on this context, the
// streaming kernels take over.
int
cg_resident_gave_up(smvs_ctx *ctx)
{
    SMVS_HIP_CHECK(hipMemsetAsync(ctx->res_work, 0, sizeof(ResExchange), ctx->stream));
    ctx->resident_disabled = true;
    return SMVS_OK;
}

int
cg_resident_enqueue(smvs_ctx *ctx, int max_iterations, double q_tolerance,
    bool test_give_up)
{
    int tag = 0, tiles = 0;
    return resident_enqueue(ctx, max_iterations, -1.0, q_tolerance, true, true,
        nullptr, &tag, &tiles, test_give_up);
}

// Returns SMVS_OK with *ran = false when the resident solver does not apply
// (grid too large for the chip, disabled, or it failed to synchronise) -- the
// caller then runs the streaming kernels.
int
cg_resident_solve(smvs_ctx *ctx, int max_iterations, double error_tolerance,
    double q_tolerance, int *num_iterations, int *info, bool *ran, bool fused)
{
    *ran = false;
    if (!cg_resident_applies(ctx, max_iterations))
        return SMVS_OK;
    // debug aid (tools/cg_trace.py): cycle stamps of workgroup 0
    static const char *trace_path = std::getenv("SMVS_CG_TRACE");
    long long *trace_dev = nullptr;
    size_t const trace_n = (size_t)TRACE_TOTAL;
    if (trace_path != nullptr) {
        SMVS_HIP_CHECK(hipMalloc((void **)&trace_dev, trace_n * sizeof(long long)));
        SMVS_HIP_CHECK(hipMemsetAsync(trace_dev, 0, trace_n * sizeof(long long),
            ctx->stream));
    }
    ScopedTileBudget guard(cg_resident_budget(ctx->device), cg_resident_tiles(ctx));
    int solve_tag = 0, num_tiles = 0;
    int const rc = resident_enqueue(ctx, max_iterations, error_tolerance,
        q_tolerance, fused, false, trace_dev, &solve_tag, &num_tiles);
    if (rc != SMVS_OK)
        return rc;

    volatile int *progress = ctx->cg_progress;
    auto const t_start = std::chrono::steady_clock::now();
    long spins = 0;
    while (__atomic_load_n(&progress[PROGRESS_DONE], __ATOMIC_ACQUIRE)
        != progress_done_word(solve_tag)) {
        __builtin_ia32_pause();
        if ((++spins & 0xFFFF) == 0) {
            hipError_t const q = hipStreamQuery(ctx->stream);
            if (q != hipSuccess && q != hipErrorNotReady)
                SMVS_HIP_CHECK(q);
            if (q == hipSuccess
                && __atomic_load_n(&progress[PROGRESS_DONE], __ATOMIC_ACQUIRE)
                    != progress_done_word(solve_tag)) {
                set_error("cg_resident_solve: kernel ended without a result");
                return SMVS_ERR_STATE;
            }
            if (std::chrono::steady_clock::now() - t_start
                > std::chrono::seconds(60)) {
                set_error("cg_resident_solve: timed out waiting for the device");
                return SMVS_ERR_STATE;
            }
        }
    }
    if (trace_dev != nullptr) {
        std::vector<long long> tr(trace_n);
        SMVS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        SMVS_HIP_CHECK(hipMemcpy(tr.data(), trace_dev, trace_n * sizeof(long long),
            hipMemcpyDeviceToHost));
        (void)hipFree(trace_dev);
        ResidentPlan plan;
        dump_trace(trace_path, tr.data(), ctx->num_nodes, num_tiles,
            progress[PROGRESS_ITERS], resident_plan(ctx, &plan) && plan.one ? 1 : 2);
    }
    // (every workgroup has passed its last barrier when the result appears:
    // the kernel is draining and cannot block a barrier kernel started now)
    if (progress[PROGRESS_GAVE_UP] != 0)
        return cg_resident_gave_up(ctx);
    ctx->last_cg_iterations = progress[PROGRESS_ITERS];
    if (num_iterations != nullptr)
        *num_iterations = progress[PROGRESS_ITERS];
    if (info != nullptr)
        *info = progress[PROGRESS_INFO];
    *ran = true;
    return SMVS_OK;
}

} // namespace smvs_hip
