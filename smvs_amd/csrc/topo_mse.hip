// mse_for_patch (lib/depth_optimizer.cc:747-790) for the patches that are
// asked about: the candidate list and the errors of its entries (topology.hip
// has the overview).
#include "topo_internal.h"
#include "topo_divide.h"

#include <cstdlib>
#include <type_traits>

namespace smvs_hip {

// ---- mse_for_patch (:747-790) ----
// Which patches are asked about: all valid ones, or (cut_boundaries) those
// with a node that has lost more than one neighbour (:401-428) -- the rim of
// the surface; the others are not evaluated (0: never above 0.05).  One thread
// per patch writes the answer of everything that is not evaluated and appends
// the rest to a list, so that the kernel doing the arithmetic is launched over
// the few per cent that need it: sixteen lanes per patch of a 129 k-patch grid
// were 32 k waves that each waited for two dependent loads to learn that they
// had nothing to do -- that, not the arithmetic, was the 35-40 us of a pass.
// (The order of the list is whatever the atomics make it; an entry's result
// does not depend on its place.)
__global__ void __launch_bounds__(256)
topo_mse_candidates_kernel(TopoArgs A)
{
    int const p = blockIdx.x * blockDim.x + threadIdx.x;
    bool const in_range = p < A.num_patches;
    bool const valid = in_range && A.patch_valid[p];
    bool alive = valid;
    if (valid && A.only_candidates) {
        int const n00 = (p / A.npx) * A.stride + p % A.npx;
        alive = (A.border_node[n00] | A.border_node[n00 + 1] | A.border_node[n00 + A.stride]
            | A.border_node[n00 + A.stride + 1]) != 0;
    }
    if (in_range && !alive)
        A.mse_out[p] = valid ? 0.0 : -1.0;
    append_listed(A, alive, p);
}

// One lane group per listed patch; the launch is bounded and a group takes
// every (number of groups)-th entry.  AT_ONCE: neighbours whose warps and
// gathers are issued together.
template <int AT_ONCE>
__global__ void __launch_bounds__(256)
topo_mse_kernel(TopoArgs A)
{
#pragma clang fp contract(off)
    __shared__ double red[4];
    int const ps = A.ps;
    int const G = group_size(ps, MSE_WORKGROUP_FROM);
    int const gl = threadIdx.x & (G - 1);
    int const g_log2 = 31 - __clz(G);
    int const group = (int)(((unsigned)blockIdx.x * blockDim.x + threadIdx.x) >> g_log2);
    int const groups = (int)(((unsigned)gridDim.x * blockDim.x) >> g_log2);
    int const count = *A.mse_count;
    // Patch sizes 32 and 64: a patch is 4 resp. 16 CHUNKS of 256 pixels, each a
    // workgroup's item of its own (round 6).  The two coarsest scales have a
    // few hundred candidates at most, so a workgroup per patch left most of the
    // chip idle behind chains of 16 pixels x 8 neighbours per lane (140-170 us
    // per launch at patch size 64).  A chunk leaves its two sums in
    // `mse_parts`; the chunk that arrives last (one atomic per chunk) adds them
    // in chunk order -- a fixed order, whichever workgroup does it -- and
    // clears the counter for the next launch.
    int const chunks = A.mse_chunks;
    // (G == 256: the group is the workgroup, its threads loop together and
    // meet in group_sum's barriers; smaller groups only shuffle among
    // themselves)
    for (int work = group; work < count * chunks; work += groups) {
        int const item = chunks > 1 ? work / chunks : work;
        int const chunk = chunks > 1 ? work - item * chunks : 0;
        int const p = A.mse_list[item];
        double n16[16];
        load_patch_nodes(A, p, n16);
        int const px = A.start_x + (p % A.npx) * ps;
        int const py = A.start_y + (p / A.npx) * ps;
        // (bits of neighbours the context does not have are not looked at)
        uint32_t const vis = A.patch_vis[p] & ((1u << A.n_subs) - 1u);
        double error = 0.0, counter = 0.0;
        int const k_begin = chunks > 1 ? chunk * 256 : 0;
        int const k_end = chunks > 1 ? k_begin + 256 : ps * ps;
        for (int k = k_begin + gl; k < k_end; k += G) {
            int const i = k & (ps - 1), j = k >> A.ps_log2;
            // (asked for before the surface is evaluated: a cold round trip)
            float2 const gm = A.main_grad[(size_t)(py + j) * A.W + (px + i)];
            // (x / ps == x * (1 / ps) exactly: ps is a power of two)
            double const u = (i + 0.5) * A.inv_ps, v = (j + 0.5) * A.inv_ps;
            double const w = smvs_topo::patch_eval(n16, u, v, 0, 0);
            double const wx = smvs_topo::patch_eval(n16, u, v, 1, 0) * A.inv_ps;
            double const wy = smvs_topo::patch_eval(n16, u, v, 0, 1) * A.inv_ps;
            double const gm0 = gm.x, gm1 = gm.y;
            // The neighbours AT_ONCE at a time: the warps, then the gathers of
            // all of them, then the sum in the neighbours' order (the few rim
            // patches this kernel is asked about make a launch as long as one
            // lane's chain of dependent divisions and gathers).
            for (int s0 = 0; s0 < A.n_subs; s0 += AT_ONCE) {
                uint32_t const some = (vis >> s0) & ((1u << AT_ONCE) - 1u);
                if (some == 0u)
                    continue;
                double jac[AT_ONCE][4];
                float g0[AT_ONCE], g1[AT_ONCE];
                auto const gather = [&](auto tag) {
#pragma unroll
                    for (int e = 0; e < AT_ONCE; ++e) {
                        // (an unseen neighbour: the first one's planes at pixel 0,
                        // loaded and not used)
                        bool const on = ((some >> e) & 1u) != 0u;
                        int const sc = on ? s0 + e : s0;
                        const double *M = A.cams->M[sc];
                        Warp wp(M, A.cams->t[sc], px + i + 0.5, py + j + 0.5, w);
                        WarpQuotients<decltype(tag)::value> const wq(wp);
                        wq.jacobian(wp, M, w, wx, wy, jac[e]);
                        float const qx = on ? (float)(wq.x(wp) - 0.5) : 0.0f;
                        float const qy = on ? (float)(wq.y(wp) - 0.5) : 0.0f;
                        SubPlanes const sp = A.subs[sc];
                        linear_at_pair(sp.grad, sp.width, sp.height, qx, qy, &g0[e], &g1[e]);
                    }
                };
                bool plain = A.exact_divisions == 0;
#pragma unroll
                for (int e = 0; e < AT_ONCE; ++e) {
                    int const sc = ((some >> e) & 1u) != 0u ? s0 + e : s0;
                    Warp wp(A.cams->M[sc], A.cams->t[sc], px + i + 0.5, py + j + 0.5, w);
                    plain = plain && WarpQuotients<true>(wp).plain();
                }
                if (plain)
                    gather(std::true_type());
                else
                    gather(std::false_type());
#pragma unroll
                for (int e = 0; e < AT_ONCE; ++e) {
                    if (((some >> e) & 1u) == 0u)
                        continue;
                    double const d0 = gm0 - (jac[e][0] * (double)g0[e] + jac[e][1] * (double)g1[e]);
                    double const d1 = gm1 - (jac[e][2] * (double)g0[e] + jac[e][3] * (double)g1[e]);
                    error += sqrt(d0 * d0 + d1 * d1);
                    counter += 1.0;
                }
            }
        }
        error = group_sum(error, G, red);
        counter = group_sum(counter, G, red);
        if (chunks == 1) {
            if (gl == 0)
                A.mse_out[p] = counter == 0.0 ? 1.0 : error / counter;
            continue;
        }
        // (chunks > 1 only with G == 256: the workgroup is the group)
        if (threadIdx.x == 0) {
            double *mine = A.mse_parts + 2 * ((size_t)item * chunks + chunk);
            __hip_atomic_store(mine, error, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(mine + 1, counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            int const before = __hip_atomic_fetch_add(A.mse_arrived + item, 1, __ATOMIC_ACQ_REL,
                __HIP_MEMORY_SCOPE_AGENT);
            if (before == chunks - 1) {
                double e = 0.0, c = 0.0;
                for (int q = 0; q < chunks; ++q) {
                    const double *part = A.mse_parts + 2 * ((size_t)item * chunks + q);
                    e += __hip_atomic_load(part, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    c += __hip_atomic_load(part + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                A.mse_out[p] = c == 0.0 ? 1.0 : e / c;
                __hip_atomic_store(A.mse_arrived + item, 0, __ATOMIC_RELAXED,
                    __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

int
prepare_patch_mse(smvs_ctx *ctx, TopoArgs *A, const char *who)
{
    if (ctx->main_grad == nullptr) {
        set_error("%s: no gradient planes", who);
        return SMVS_ERR_STATE;
    }
    for (int j = 0; j < ctx->n_subs; ++j)
        if (!((ctx->planes_ok >> j) & 1u)) {
            set_error("%s: sub view %d has no planes", who, j);
            return SMVS_ERR_STATE;
        }
    int rc;
    if ((rc = device_grow(&ctx->topo_mse, &ctx->topo_mse_cap, (size_t)ctx->num_patches)) != SMVS_OK)
        return rc;
    if ((rc = device_grow(&ctx->topo_border, &ctx->topo_border_cap, (size_t)ctx->num_nodes))
        != SMVS_OK)
        return rc;
    if ((rc = device_grow(&ctx->topo_mse_list, &ctx->topo_mse_list_cap, (size_t)ctx->num_patches))
        != SMVS_OK)
        return rc;
    // patch sizes 32 and up: the kernel works in chunks of 256 pixels
    int const pp = ctx->patchsize * ctx->patchsize;
    int const chunks = group_size(ctx->patchsize, MSE_WORKGROUP_FROM) == 256
        && pp > 256 ? pp / 256 : 1;
    if (chunks > 1) {
        size_t const parts = (size_t)ctx->num_patches * chunks * 2;
        if ((rc = device_grow(&ctx->topo_mse_parts, &ctx->topo_mse_parts_cap, parts)) != SMVS_OK)
            return rc;
        size_t const had = ctx->topo_mse_arrived_cap;
        if ((rc = device_grow(&ctx->topo_mse_arrived, &ctx->topo_mse_arrived_cap,
                 (size_t)ctx->num_patches)) != SMVS_OK)
            return rc;
        if (ctx->topo_mse_arrived_cap != had)   // (a new buffer: the counters start at zero)
            SMVS_HIP_CHECK(hipMemsetAsync(ctx->topo_mse_arrived, 0,
                sizeof(int) * (size_t)ctx->num_patches, ctx->stream));
    }
    rc = fill_args(ctx, A, who);
    A->mse_chunks = chunks;
    A->mse_parts = ctx->topo_mse_parts;
    A->mse_arrived = ctx->topo_mse_arrived;
    return rc;
}

// The candidate list, then the errors of its entries.  count_is_zero: the
// caller has cleared I_TOPO_CANDIDATES on the stream (with its own words).
int
launch_patch_mse(smvs_ctx *ctx, TopoArgs const &A, bool count_is_zero)
{
    if (!count_is_zero)
        SMVS_HIP_CHECK(hipMemsetAsync(ctx->status + I_TOPO_CANDIDATES, 0, sizeof(int),
            ctx->stream));
    hipLaunchKernelGGL(topo_mse_candidates_kernel,
        dim3((unsigned)((ctx->num_patches + 255) / 256)), dim3(256), 0, ctx->stream, A);
    return launch_patch_mse_listed(ctx, A);
}

// The errors of the patches on the list (the candidates are on the stream).
int
launch_patch_mse_listed(smvs_ctx *ctx, TopoArgs const &A)
{
    // enough groups for every CU to hold its fill of waves, never more than the
    // patches: a group walks the list with that stride
    long long const group = group_size(ctx->patchsize, MSE_WORKGROUP_FROM);
    long long const items = (long long)ctx->num_patches * group * A.mse_chunks;
    long long blocks = (items + 255) / 256;
    if (blocks > 1024)
        blocks = 1024;
    // SMVS_MSE_SUBS=1: the neighbours of a pixel one after the other (eight at
    // a time measured slower than four: 34 against 31 us)
    const char *subs = std::getenv("SMVS_MSE_SUBS");
    if (subs != nullptr && std::atoi(subs) == 1)
        hipLaunchKernelGGL(topo_mse_kernel<1>, dim3((unsigned)blocks), dim3(256), 0,
            ctx->stream, A);
    else
        hipLaunchKernelGGL(topo_mse_kernel<4>, dim3((unsigned)blocks), dim3(256), 0,
            ctx->stream, A);
    SMVS_HIP_CHECK(hipGetLastError());
    return SMVS_OK;
}

} // namespace smvs_hip

using namespace smvs_hip;

extern "C" int
smvs_topology_patch_mse(smvs_ctx *ctx, double *mse_out)
{
    SMVS_REQUIRE(ctx && mse_out, "null argument");
    SMVS_HIP_CHECK(set_device(ctx->device));
    TopoArgs A;
    int rc = prepare_patch_mse(ctx, &A, "smvs_topology_patch_mse");
    if (rc == SMVS_OK)
        rc = launch_patch_mse(ctx, A, false);
    if (rc != SMVS_OK)
        return rc;
    SMVS_HIP_CHECK(hipMemcpyAsync(mse_out, ctx->topo_mse,
        sizeof(double) * ctx->num_patches, hipMemcpyDeviceToHost, ctx->stream));
    SMVS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return SMVS_OK;
}
