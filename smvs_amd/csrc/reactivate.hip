// Re-activation and the end of a Newton step, kernels and launchers
// (newton_step.h): DepthOptimizer::fill_node_reprojections (reference:
// lib/depth_optimizer.cc:647-677), Surface::update_nodes (lib/surface.cc:957-981)
// and the active-set test (lib/depth_optimizer.cc:275-303).
#include "newton_step.h"
#include "patch_bicubic.h"

namespace smvs_hip {

struct ReactivateArgs {
    const double *nodes;
    const double *x;            // delta
    const uint8_t *patch_valid;
    const uint32_t *patch_vis;
    const uint8_t *active;
    uint8_t *active_next;
    const double *hermite_tab;
    const DeviceCameras *cams;
    double *partials;
    double *scalars;
    int *status;
    int npx, stride, ps, start_x, start_y, n_subs, num_patches;
    int ps_log2;            // ps = 1 << ps_log2 (Surface: patchsize = 2^scale)
    double threshold;
    int full_optimization;
    const int *live_list;   // the step's live patches, or nullptr: all patches
    int live_count;
    int check_stop;
};

// One pixel (u, v) against one neighbour: did its reprojection move by more
// than the threshold (th2 = threshold^2); FULL: the shift itself is added to
// *sum.
//   (w0 p + t0)/(w0 r + t2) - (w1 p + t0)/(w1 r + t2)
//     = (w0 - w1)(p t2 - r t0) / ((w0 r + t2)(w1 r + t2)):
// no cancellation; the numerators are affine in the pixel
// (depth_optimizer.cc:669-672, 277-303).
// The comparison decides an active set, so the roundings are part of the
// result: the source fixes which product fuses with which sum (contraction
// off, the FMAs written out) instead of leaving it to the compiler, whose
// choice follows the shape of the surrounding code -- with several pixels of
// one column per thread M[6] * u has several uses and would no longer be the
// product that fuses.  These are the fusions of the one-pixel kernel of
// rounds 1-6 as compiled (read from its instruction sequence):
//   r = fma(M6, u, M7 v) + M8, likewise nx and ny; den = fma(w0, r, t2) *
//   fma(w1, r, t2); nx^2 + ny^2 = fma(nx, nx, ny ny).
template <bool FULL>
__device__ __forceinline__ bool
pixel_moved(const double *M, const double *t, const double *sh, double u, double v,
    double w0, double w1, double dw, double th2, double *sum)
{
#pragma clang fp contract(off)
    double const r = __builtin_fma(M[6], u, M[7] * v) + M[8];
    double const nx = __builtin_fma(sh[0], u, sh[1] * v) + sh[2];
    double const ny = __builtin_fma(sh[3], u, sh[4] * v) + sh[5];
    double const den = __builtin_fma(w0, r, t[2]) * __builtin_fma(w1, r, t[2]);
    double const num2 = (dw * dw) * __builtin_fma(nx, nx, ny * ny);
    if (FULL) {
        // the mean shift needs the quotient itself
        double inv = __builtin_amdgcn_rcp(den);
        inv = __builtin_fma(__builtin_fma(-den, inv, 1.0), inv, inv);
        inv = __builtin_fma(__builtin_fma(-den, inv, 1.0), inv, inv);
        double const d2 = num2 * inv * inv;
        *sum += sqrt(d2);
        return d2 > th2;
    }
    // shift^2 > threshold^2 without the division
    return num2 > th2 * (den * den);
}

// One thread per (patch, column ci, K consecutive rows) of the
// full-resolution pixels: project with the old and the updated nodes into
// every visible neighbour (pixel coordinates WITHOUT the +0.5 convention,
// depth_optimizer.cc:669-672).  A patch has ps^2 / K threads; K <= ps.
// What the K pixels of a thread share is done once: the patch record (32
// doubles, 16 vector loads), the x-direction sums of the bicubic
// (eval_patch_column) and the walk over the neighbours with its scalar loads
// of the camera words.  Inside the walk the K pixel tests do not depend on
// one another, but as compiled they run one after the other through the same
// registers: the saving is the shared loads, x-direction FMAs and scalar work
// and the four times fewer waves, not an overlap of the K tests.
// FULL: DepthOptimizer::Options::full_optimization (the mean shift instead of
// the active set, depth_optimizer.cc:277-288).  A template argument since round
// 6: as a run-time flag the compiler evaluated BOTH variants of the test for
// every neighbour and selected (38 FP64 instructions per neighbour where the
// active-set test needs 20).
// Without FULL the result (the flags) does not depend on K: every pixel's test
// has the bits of the one-pixel kernel.  With FULL a thread adds its K pixels'
// shifts before the wave and workgroup sums, so the association of the mean's
// sum changes with K in the last bits -- as it already does from run to run:
// the workgroups' sums meet in atomics, and the mean is only compared with
// the 0.01 threshold.
template <bool FULL, int K>
__global__ void __launch_bounds__(256)
reactivate_kernel(ReactivateArgs A)
{
    static_assert(K == 1 || K == 2 || K == 4, "rows per thread");
    constexpr int LOG2K = K == 4 ? 2 : K == 2 ? 1 : 0;
    long long const gid0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    // (the wave-uniform words every thread needs first, asked for together: as
    // three tests in a row they were three scalar round trips before a wave's
    // first vector load)
    int const stop_words = A.status[I_STOP] | A.status[I_STEP_ABORT];
    int const live_on_device = A.status[I_LIVE_PATCHES];
    double const x0 = A.x[0];
    // the pipelined Newton loop: the loop has already ended / the solver of
    // this step gave up (finish_step_kernel reports it)
    if (A.check_stop && stop_words != 0)
        return;
    // the list length is read on the device when the launch was sized before
    // it was known (live_count < 0)
    int const live_count = A.live_list == nullptr ? A.num_patches
        : (A.live_count >= 0 ? A.live_count : live_on_device);
    // threads of a patch: ps^2 / K (the patch size is a power of two: shifts
    // instead of 64-bit divisions, which cost more than the arithmetic of a
    // pixel)
    int const tshift = 2 * A.ps_log2 - LOG2K;
    if (((long long)live_count << tshift) > (long long)gridDim.x * blockDim.x) {
        // (cannot happen behind a patch kernel of the same step, which is
        // sized for the same length and would have abandoned the step)
        if (gid0 == 0)
            A.status[I_STEP_ABORT] = ABORT_GRID;
        return;
    }
    // NaN guard of the reference on delta[0] (depth_optimizer.cc:267)
    if (isnan(x0))
        return;
    int const slot = (int)(gid0 >> tshift);
    int const tid = (int)(gid0 & (long long)((1 << tshift) - 1));
    // Round 6: ONE level of dependent loads behind the list entry (before: list
    // entry -> validity -> active flags -> nodes and deltas -> visibility mask):
    // everything that depends only on the patch id is asked for at once, whether
    // or not the patch turns out to need evaluation.
    int patch = -1;
    if (slot < live_count)
        patch = A.live_list != nullptr ? A.live_list[slot] : slot;
    bool const in_range = patch >= 0 && patch < A.num_patches;
    int const pc = in_range ? patch : 0;
    int const ix = pc % A.npx, iy = pc / A.npx;
    int const n00 = iy * A.stride + ix;
    int const ids[4] = { n00, n00 + 1, n00 + A.stride, n00 + A.stride + 1 };
    uint8_t const valid = A.patch_valid[pc];
    uint8_t const act = A.active[ids[0]] | A.active[ids[1]] | A.active[ids[2]]
        | A.active[ids[3]];
    uint32_t const vis = A.patch_vis[pc];
    // w1 - w0 is the patch evaluated on the node deltas (the patch
    // is linear in its nodes)
    double th0[16], thd[16];
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            th0[4 * n + k] = A.nodes[4 * (size_t)ids[n] + k];
            thd[4 * n + k] = A.x[4 * (size_t)ids[n] + k];
        }
    double sum = 0.0, cnt = 0.0;
    bool moved = false;
    if (in_range && valid && act != 0) {
        double const th2 = A.threshold * A.threshold;
        int const ci = tid & (A.ps - 1), cj0 = (tid >> A.ps_log2) << LOG2K;
        double g0[4], gd[4];
        eval_patch_column(A.hermite_tab, ci, th0, g0);
        eval_patch_column(A.hermite_tab, ci, thd, gd);
        double w0[K], w1[K], dw[K], v[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            w0[k] = eval_patch_row(A.hermite_tab, cj0 + k, g0);
            dw[k] = eval_patch_row(A.hermite_tab, cj0 + k, gd);
            w1[k] = w0[k] + dw[k];
            v[k] = (double)(A.start_y + iy * A.ps + cj0 + k);
        }
        double const u = (double)(A.start_x + ix * A.ps + ci);
        for (int j = 0; j < A.n_subs; ++j) {
            if (!((vis >> j) & 1u))
                continue;
            const double *M = A.cams->M[j];
            const double *t = A.cams->t[j];
            const double *sh = A.cams->shift[j];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                cnt += 1.0;
                moved |= pixel_moved<FULL>(M, t, sh, u, v[k], w0[k], w1[k], dw[k],
                    th2, &sum);
            }
        }
    }
    if (!FULL) {
        // One lane per patch and wave raises the four flags (rounds 1-5: every
        // pixel that moved wrote them -- in a first step nearly all of 2 M
        // threads, four byte stores each to 128 k distinct bytes).  The lanes of
        // a patch are an aligned group of min(64, ps^2 / K): they share the patch
        // and its node ids.
        int const lane = (int)(threadIdx.x & 63u);
        int const group = tshift >= 6 ? 64 : 1 << tshift;
        unsigned long long const votes = __ballot(moved);
        unsigned long long const mine = group >= 64 ? ~0ull
            : ((1ull << group) - 1ull) << (lane & ~(group - 1));
        if ((votes & mine) != 0ull && (lane & (group - 1)) == 0) {
            A.active_next[ids[0]] = 1;
            A.active_next[ids[1]] = 1;
            A.active_next[ids[2]] = 1;
            A.active_next[ids[3]] = 1;
        }
    }
    if (!FULL)
        return;
    // mean reprojection delta (depth_optimizer.cc:277-282)
    __shared__ double red[2][4];
    int const lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        sum += __shfl_xor(sum, off);
        cnt += __shfl_xor(cnt, off);
    }
    if (lane == 0) {
        red[0][wave] = sum;
        red[1][wave] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0, c = 0.0;
        for (int wv = 0; wv < 4; ++wv) {
            s += red[0][wv];
            c += red[1][wv];
        }
        // the number of blocks can exceed the CG partial buffer: accumulate
        // with atomics (order-dependent in the last bits; only compared
        // against the 0.01 threshold).
        atomicAdd(&A.scalars[S_SUMDIFF], s);
        atomicAdd(&A.scalars[S_COUNT_DIFF], c);
    }
}

// Pixels per thread of reactivate_kernel at patch size 2^ps_log2: four at every
// scale, never more than the patch has rows.  Measured per launch on MI355X
// (1920 x 1080, 8 neighbours, the Newton loops of one optimize(), scales 2 / 3 /
// 4 / 5 / 6; profiles/reactivate_after.txt):
//   one pixel per thread (rounds 1-6)   33 / 31 / 30 / 23 / 17 us
//   one, this kernel with K = 1         36 / 33 / 32 / 24 / 19 us
//   two                                 24 / 23 / 22 / 17 / 13 us
//   four                                22 / 21 / 19 / 15.5 / 12.5 us
// and sixteen (one thread per 4 x 4 chunk, round 6) 40 us where one took 25:
// too few waves to hide the latency of its serial pixels.  With one pixel per
// thread a wave lived 11,300 cycles and issued during 16 % of them
// (profiles/reactivate_before.txt); staging the patch records of a workgroup in
// LDS changed nothing then (round 6) and was not tried again.  Not tried on top
// of four pixels: wave-uniform loads of the patch record where a whole wave
// shares a patch, the neighbours' camera words staged once per workgroup.
// SMVS_REACTIVATE_PIXELS=1|2|4 (read once) forces one value for every scale:
// tests/test_gpu_reactivate_pixels.py runs each, and it is the A/B switch of
// the table above.
static int
reactivate_pixels(int ps_log2)
{
    static int const forced = [] {
        const char *e = std::getenv("SMVS_REACTIVATE_PIXELS");
        int const k = e != nullptr ? std::atoi(e) : 0;
        return k == 1 || k == 2 || k == 4 ? k : 0;
    }();
    int k = forced != 0 ? forced : 4;
    while (k > (1 << ps_log2))
        k >>= 1;
    return k;
}

// delta[0] NaN guard (depth_optimizer.cc:267-268) and reset of the next set
__global__ void
prepare_update_kernel(uint8_t *active_next, int num_nodes, double *scalars,
    int *status)
{
    int const i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < num_nodes)
        active_next[i] = 0;
    if (i == 0) {
        status[I_NUM_ACTIVE] = 0;
        scalars[S_SUMDIFF] = 0.0;
        scalars[S_COUNT_DIFF] = 0.0;
    }
}

// nodes += delta for valid nodes (surface.cc:964-975); adopt the new active
// set and count it (depth_optimizer.cc:291-303).
__global__ void
apply_update_kernel(double *nodes, const double *x, const uint8_t *node_valid,
    uint8_t *active, const uint8_t *active_next, int num_nodes,
    int full_optimization, int *status)
{
    bool const skip = isnan(x[0]);
    int const i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0)
        status[I_NAN] = skip ? 1 : 0;
    bool on = false;
    if (!skip && i < num_nodes) {
        if (node_valid[i]) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                nodes[4 * (size_t)i + k] += x[4 * (size_t)i + k];
        }
        if (!full_optimization) {
            active[i] = active_next[i];
            on = active_next[i] == 1;
        } else {
            on = active[i] == 1;
        }
    }
    int const cnt = __syncthreads_count(on);
    if (threadIdx.x == 0 && cnt != 0)
        atomicAdd(&status[I_NUM_ACTIVE], cnt);
}

// End of a Newton step inside smvs_gn_run_loop, one launch instead of node
// update + list build + two device-to-host copies: thread c owns node c
// (nodes += delta, adopt the new active flag, count it, surface.cc:957-981,
// depth_optimizer.cc:291-303) and, where c is also the top-left node of a
// patch, that patch's entry in the next step's live list.  The last
// workgroup to finish publishes the step's result words in pinned host
// memory, which the host polls (no stream query, no copies).
struct FinishArgs {
    double *nodes;
    const double *x;
    const uint8_t *node_valid;
    const uint8_t *patch_valid;
    uint8_t *active;
    const uint8_t *active_next;
    int *list;
    int *status;
    unsigned long long *counter;   // bits 0-23 list length, 24-47 active nodes,
                                   // 48-63 workgroups arrived: ONE atomic per workgroup
                                   // (wide: [0] = list length | active nodes << 32,
                                   // [1] = workgroups arrived)
    int wide;              // surfaces of 2^24 nodes and more: two atomics per workgroup
    const double *scalars;
    int *host_words;       // pinned slot of the step (newton_step.h, STEP_*)
    int npx, npy, stride, num_nodes;
    int full_optimization;
    int seq;
    int check_stop;        // launch-ahead mode: obey / maintain status[I_STOP]
    double full_opt_threshold;
    int begin;             // 1: the start of a loop instead of the end of a step --
                           // no node update; count the active set into
                           // status[I_NUM_INITIAL], build the first live list,
                           // clear the stop / abort words
    int reset_active;      // begin: active := valid nodes first (surface.cc:37-44)
};

constexpr int FINISH_THREADS = 1024;

__global__ void __launch_bounds__(FINISH_THREADS)
finish_step_kernel(FinishArgs A)
{
    if (A.check_stop && !A.begin) {
        // enqueued before the loop was known to have ended / the solver to
        // have given up: report it, touch nothing
        int const abort = A.status[I_STEP_ABORT];
        int const gate = A.status[I_STOP] != 0 ? GATE_SKIPPED
            : (abort != 0 ? GATE_ABANDONED + abort : GATE_RAN);
        if (gate != GATE_RAN) {
            if (blockIdx.x == 0 && threadIdx.x == 0) {
                __hip_atomic_store(A.host_words + STEP_GATE, gate, __ATOMIC_RELAXED,
                    __HIP_MEMORY_SCOPE_SYSTEM);
                __hip_atomic_store(A.host_words + STEP_SEQ, A.seq, __ATOMIC_RELEASE,
                    __HIP_MEMORY_SCOPE_SYSTEM);
            }
            return;
        }
    }
    bool const begin = A.begin != 0;
    // depth_optimizer.cc:267: nothing is updated
    bool const skip = begin ? false : isnan(A.x[0]);
    bool const keep = begin ? A.reset_active == 0 : (skip || A.full_optimization != 0);
    // the flags the new active set comes from when it is not kept
    const uint8_t *incoming = begin ? A.node_valid : A.active_next;
    int const c = blockIdx.x * blockDim.x + threadIdx.x;
    bool on = false, live = false;
    int patch = 0;
    if (c < A.num_nodes) {
        if (!begin && !skip && A.node_valid[c]) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                A.nodes[4 * (size_t)c + k] += A.x[4 * (size_t)c + k];
        }
        // (other threads read `incoming`, never the flag adopted here)
        uint8_t const flag = keep ? A.active[c] : (incoming[c] != 0 ? 1 : 0);
        if (!keep)
            A.active[c] = flag;
        on = flag == 1;
        int const ix = c % A.stride, iy = c / A.stride;
        if (ix < A.npx && iy < A.npy) {
            patch = iy * A.npx + ix;
            const uint8_t *f = keep ? A.active : incoming;
            live = A.patch_valid[patch]
                && (flag | f[c + 1] | f[c + A.stride] | f[c + A.stride + 1]) != 0;
        }
    }
    // What the publishing thread reports besides the counts was written by
    // earlier launches of the stream: asked for here, all at once, instead of
    // one dependent round trip after the other behind the atomics (a launch of
    // ONE workgroup took 8.5 us, most of it that chain).
    int pre_active_patches = 0, pre_initial = 0, pre_iter = 0;
    double pre_sum_diff = 0.0, pre_count_diff = 0.0;
    if (threadIdx.x == 0) {
        pre_active_patches = A.status[I_ACTIVE_PATCHES];
        pre_initial = A.status[I_NUM_INITIAL];
        pre_iter = A.status[I_ITER];
        pre_sum_diff = A.scalars[S_SUMDIFF];
        pre_count_diff = A.scalars[S_COUNT_DIFF];
    }
    constexpr int WAVES = FINISH_THREADS / 64;
    __shared__ int wave_cnt[WAVES];
    __shared__ int base;
    __shared__ unsigned long long seen;
    __shared__ bool last_wide;
    int const lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long const ballot = __ballot(live);
    int const before = __popcll(ballot & ((1ull << lane) - 1ull));
    if (lane == 0)
        wave_cnt[wave] = __popcll(ballot);
    int const cnt_on = __syncthreads_count(on);
    if (threadIdx.x == 0) {
        int total = 0;
        for (int wv = 0; wv < WAVES; ++wv)
            total += wave_cnt[wv];
        // one device-scope atomic per workgroup (atomics on one address are
        // served one after the other): list slots, active nodes and arrival
        if (!A.wide) {
            unsigned long long const add = (unsigned long long)total
                | ((unsigned long long)cnt_on << 24) | (1ull << 48);
            unsigned long long const old = atomicAdd(A.counter, add);
            base = (int)(old & 0xFFFFFFull);
            seen = old + add;
        } else {
            // the counts no longer fit beside the arrivals: the counts first,
            // then the arrival as a release / acquire (the counts of every
            // workgroup whose arrival the last one observes are visible to
            // its read-back); the last arriver reads the totals back
            unsigned long long const add = (unsigned long long)total
                | ((unsigned long long)cnt_on << 32);
            unsigned long long const old = atomicAdd(A.counter, add);
            base = (int)(old & 0xFFFFFFFFull);
            unsigned long long const arrived = __hip_atomic_fetch_add(A.counter + 1, 1ull,
                __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) + 1ull;
            unsigned long long totals = 0ull;
            if (arrived == (unsigned long long)gridDim.x)
                totals = __hip_atomic_fetch_add(A.counter, 0ull, __ATOMIC_ACQUIRE,
                    __HIP_MEMORY_SCOPE_AGENT);
            // same layout as the packed word: length, active nodes, arrivals
            // (the packed fields are only decoded below)
            seen = arrived == (unsigned long long)gridDim.x ? totals : 0ull;
            last_wide = arrived == (unsigned long long)gridDim.x;
        }
    }
    __syncthreads();
    if (live) {
        int off = base + before;
        for (int wv = 0; wv < wave; ++wv)
            off += wave_cnt[wv];
        A.list[off] = patch;
    }
    // the workgroup that arrives last publishes the step (no fences: the
    // counters travelled in the atomic itself)
    bool const last = A.wide ? last_wide
        : (seen >> 48) == (unsigned long long)gridDim.x;
    if (threadIdx.x == 0 && last) {
        int const next_live = A.wide ? (int)(seen & 0xFFFFFFFFull)
            : (int)(seen & 0xFFFFFFull);
        int const num_active = A.wide ? (int)(seen >> 32)
            : (int)((seen >> 24) & 0xFFFFFFull);
        A.counter[0] = 0ull;   // (nobody else touches them any more) for the next launch
        A.counter[1] = 0ull;
        // (the publishing workgroup is whichever arrives last; thread 0 of
        // every workgroup has asked for the same words)
        int active_patches = pre_active_patches, initial = pre_initial;
        if (begin) {
            A.status[I_NUM_INITIAL] = num_active;
            A.status[I_STEP_ABORT] = 0;
            A.status[I_ACTIVE_PATCHES] = 0;
            active_patches = 0;
            initial = num_active;
        }
        A.status[I_NAN] = skip ? 1 : 0;
        A.status[I_NUM_ACTIVE] = num_active;
        A.status[I_LIVE_PATCHES] = next_live;
        __hip_atomic_store(A.host_words + STEP_NUM_ACTIVE, num_active, __ATOMIC_RELAXED,
            __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(A.host_words + STEP_NAN, skip ? 1 : 0, __ATOMIC_RELAXED,
            __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(A.host_words + STEP_ACTIVE_PATCHES, active_patches,
            __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(A.host_words + STEP_NEXT_LIVE, next_live, __ATOMIC_RELAXED,
            __HIP_MEMORY_SCOPE_SYSTEM);
        double const sum_diff = pre_sum_diff;
        double const count_diff = pre_count_diff;
        // does the loop go on?  (depth_optimizer.cc:219-220, 267-268, 277-288;
        // the step limit is the host's business)
        bool stop = skip;
        if (A.full_optimization && !begin)
            stop = stop || sum_diff / count_diff < A.full_opt_threshold;
        else
            stop = stop || !(num_active > initial / 20);
        if (A.check_stop || begin)
            A.status[I_STOP] = stop ? 1 : 0;
        __hip_atomic_store(A.host_words + STEP_GATE, GATE_RAN, __ATOMIC_RELAXED,
            __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(A.host_words + STEP_CG_ITERS, begin ? 0 : pre_iter, __ATOMIC_RELAXED,
            __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(A.host_words + STEP_LOOP_ENDS, stop ? 1 : 0, __ATOMIC_RELAXED,
            __HIP_MEMORY_SCOPE_SYSTEM);
        double *host_scalars = reinterpret_cast<double *>(A.host_words + STEP_SCALARS);
        host_scalars[0] = sum_diff;
        host_scalars[1] = count_diff;
        __hip_atomic_store(A.host_words + STEP_SEQ, A.seq, __ATOMIC_RELEASE,
            __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

static FinishArgs
finish_args(smvs_ctx *ctx, int seq)
{
    FinishArgs F = {};   // the mode words zero: the end of a step, not enqueued ahead
    F.nodes = ctx->nodes;
    F.x = ctx->x;
    F.node_valid = ctx->node_valid;
    F.patch_valid = ctx->patch_valid;
    F.active = ctx->active;
    F.active_next = ctx->active_next;
    F.list = ctx->live_list;
    F.status = ctx->status;
    F.counter = ctx->step_counter;
    F.scalars = ctx->scalars;
    F.host_words = step_slot(ctx, seq);
    F.npx = ctx->npx;
    F.npy = ctx->npy;
    F.stride = ctx->node_stride;
    F.num_nodes = ctx->num_nodes;
    F.wide = ctx->num_nodes >= (1 << 24) || loop_test_mode() == LOOP_TEST_WIDE ? 1 : 0;
    F.seq = seq;
    return F;
}

static int
finish_launch(smvs_ctx *ctx, FinishArgs const &F)
{
    ScopedKernelTimer timer(ctx, SMVS_K_MISC);
    hipLaunchKernelGGL(finish_step_kernel,
        dim3((unsigned)((ctx->num_nodes + FINISH_THREADS - 1) / FINISH_THREADS)),
        dim3(FINISH_THREADS), 0, ctx->stream, F);
    SMVS_HIP_CHECK(hipGetLastError());
    return SMVS_OK;
}

int
loop_begin_launch(smvs_ctx *ctx, bool reset_active, int seq)
{
    FinishArgs F = finish_args(ctx, seq);
    F.begin = 1;
    F.reset_active = reset_active ? 1 : 0;
    if (reset_active)
        ctx->cg_use_active = false;   // as smvs_ctx_set_active
    return finish_launch(ctx, F);
}

// prepare_update_kernel unless the flags are clear already, reactivate_kernel
// over `live` entries of the live list (negative: no list, every patch); ahead:
// only sized for `live`, the length and the stop words are read on the device.
static int
reactivate_kernel_launch(smvs_ctx *ctx, double threshold, int full_optimization,
    int live, bool ahead)
{
    int const N = ctx->num_nodes;
    // (the assembly kernel of the same Newton step has already cleared the
    // flags and counters when the system came from smvs_gn_construct)
    if (!ctx->update_prepared) {
        ScopedKernelTimer timer(ctx, SMVS_K_MISC);
        hipLaunchKernelGGL(prepare_update_kernel, dim3((unsigned)((N + 255) / 256)),
            dim3(256), 0, ctx->stream, ctx->active_next, N, ctx->scalars,
            ctx->status);
    }
    ctx->update_prepared = false;
    SMVS_HIP_CHECK(hipGetLastError());
    ReactivateArgs A;
    A.nodes = ctx->nodes;
    A.x = ctx->x;
    A.patch_valid = ctx->patch_valid;
    A.patch_vis = ctx->patch_vis;
    A.active = ctx->active;
    A.active_next = ctx->active_next;
    A.hermite_tab = ctx->hermite_tab;
    A.cams = ctx->cams;
    A.partials = ctx->partials;
    A.scalars = ctx->scalars;
    A.status = ctx->status;
    A.npx = ctx->npx;
    A.stride = ctx->node_stride;
    A.ps = ctx->patchsize;
    A.ps_log2 = ctx->scale;
    A.start_x = ctx->start_x;
    A.start_y = ctx->start_y;
    A.n_subs = ctx->n_subs;
    A.num_patches = ctx->num_patches;
    A.threshold = threshold;
    A.full_optimization = full_optimization;
    // the live list of this step (built at the end of the previous one) when
    // the host knows its length
    A.live_list = live >= 0 ? ctx->live_list : nullptr;
    A.live_count = ahead ? -1 : live;   // -1: read on the device
    A.check_stop = ahead ? 1 : 0;
    // ps^2 / K threads per patch of the list (or of the surface)
    int const K = reactivate_pixels(ctx->scale);
    long long const items = (long long)(live >= 0 ? live
        : ctx->num_patches) * ctx->patchsize * ctx->patchsize / K;
    {
        ScopedKernelTimer timer(ctx, SMVS_K_REACTIVATE);
        dim3 const grid((unsigned)((items + 255) / 256 > 0 ? (items + 255) / 256 : 1));
        void (*kernel)(ReactivateArgs) = full_optimization
            ? (K == 4 ? reactivate_kernel<true, 4> : K == 2 ? reactivate_kernel<true, 2>
                : reactivate_kernel<true, 1>)
            : (K == 4 ? reactivate_kernel<false, 4> : K == 2 ? reactivate_kernel<false, 2>
                : reactivate_kernel<false, 1>);
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, ctx->stream, A);
    }
    SMVS_HIP_CHECK(hipGetLastError());
    return SMVS_OK;
}

int
reactivate_launch(smvs_ctx *ctx, double threshold, int full_optimization)
{
    int const rc = reactivate_kernel_launch(ctx, threshold, full_optimization, -1, false);
    if (rc != SMVS_OK)
        return rc;
    int const N = ctx->num_nodes;
    ScopedKernelTimer timer(ctx, SMVS_K_MISC);
    hipLaunchKernelGGL(apply_update_kernel, dim3((unsigned)((N + 255) / 256)),
        dim3(256), 0, ctx->stream, ctx->nodes, ctx->x, ctx->node_valid,
        ctx->active, ctx->active_next, N, full_optimization, ctx->status);
    SMVS_HIP_CHECK(hipGetLastError());
    return SMVS_OK;
}

int
step_end_launch(smvs_ctx *ctx, double threshold, int full_optimization,
    StepEnd const &E)
{
    int const rc = reactivate_kernel_launch(ctx, threshold, full_optimization, E.live,
        E.ahead);
    if (rc != SMVS_OK)
        return rc;
    // node update, next live list and the result words in one launch
    FinishArgs F = finish_args(ctx, E.seq);
    F.full_optimization = full_optimization;
    F.check_stop = E.ahead ? 1 : 0;
    F.full_opt_threshold = E.ahead ? E.full_opt_threshold : 0.0;
    return finish_launch(ctx, F);
}

} // namespace smvs_hip

using namespace smvs_hip;

extern "C" int
smvs_update_and_reactivate(smvs_ctx *ctx, double threshold,
    int full_optimization, int *num_active, double *mean_delta, int *nan_flag)
{
    SMVS_REQUIRE(ctx != nullptr, "null context");
    if (!ctx->has_surface || !ctx->has_cameras) {
        set_error("smvs_update_and_reactivate: no surface / cameras");
        return SMVS_ERR_STATE;
    }
    SMVS_HIP_CHECK(set_device(ctx->device));
    int rc = reactivate_launch(ctx, threshold, full_optimization);
    if (rc != SMVS_OK)
        return rc;
    SMVS_HIP_CHECK(hipMemcpyAsync(ctx->status_host, ctx->status,
        sizeof(int) * I_NUM, hipMemcpyDeviceToHost, ctx->stream));
    SMVS_HIP_CHECK(hipMemcpyAsync(ctx->scalars_host, ctx->scalars,
        sizeof(double) * S_NUM, hipMemcpyDeviceToHost, ctx->stream));
    SMVS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (num_active != nullptr)
        *num_active = ctx->status_host[I_NUM_ACTIVE];
    if (nan_flag != nullptr)
        *nan_flag = ctx->status_host[I_NAN];
    // sum / count like depth_optimizer.cc:277-282: NaN when no patch is seen
    // by any neighbour (0 / 0), which the caller's `update < 0.01` rejects
    if (mean_delta != nullptr)
        *mean_delta = ctx->scalars_host[S_SUMDIFF]
            / ctx->scalars_host[S_COUNT_DIFF];
    return SMVS_OK;
}
