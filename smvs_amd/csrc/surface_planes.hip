// Node slopes from the SGM plane hypotheses (include/smvs_hip.h, "Node slopes
// from the SGM plane hypotheses"; not in the reference, opt-in): the slant
// plane of a context -- the SGM front end's slants tapped to full resolution
// -- and initialize_node_from_depth with it for the surface of
// smvs_surface_create_planes.  The per-element arithmetic is
// csrc/host/surface_math.h's (slant_tap, slant_key, node_from_window_planes),
// which the host mirror compiles too.  surface.hip keeps the reference's
// kernel and every entry point of the surgery; it calls
// launch_init_nodes_planes while the surface holds a slant plane.
#include "common.h"

#include "host/surface_math.h"

namespace smvs_hip {

using smvs_surf::Grid;

// ---- the slant plane: one lane per full-resolution pixel ----
struct SlantTapArgs {
    const float *lowres;     // L [dm_h][dm_w]
    const float *slant;      // G [dm_h][dm_w][2]
    float2 *plane;           // P [h][w]
    int dm_w, dm_h, w, h;
};

__global__ void __launch_bounds__(256)
surf_slant_tap_kernel(SlantTapArgs A)
{
#pragma clang fp contract(off)
    size_t const i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)A.w * A.h)
        return;
    int const y = (int)(i / (size_t)A.w), x = (int)(i - (size_t)y * A.w);
    float p[2];
    smvs_surf::slant_tap(A.lowres, A.slant, A.dm_w, A.dm_h, A.w, A.h, x, y, p);
    A.plane[i] = make_float2(p[0], p[1]);
}

// ---- initialize_node_from_depth with slants for every null node ----
// The shape of surf_init_nodes_kernel (surface.hip): one lane group of
// G = min(64, ps^2) lanes per node, the window's ps^2 pixels dealt to the
// lanes, E = ps^2 / G per lane.  Three rank selections, one after the other:
// the depth (31 passes over the positive keys, the parent's loop), then the
// first and the second slant component (32 passes each over the signed keys of
// the members of S).  Membership in S is decided when the window is loaded --
// a positive depth and two finite components -- and travels with the keys: a
// non-member holds NO_SLANT, the key of a NaN, which no finite float has.
//
// Registers: a lane keeps its E depth keys (CACHE of them, as the parent) and
// ONE array of E slant keys.  The array holds the first component through
// the load, the count of S and the first selection; the second component is
// then loaded over it (one more read of the plane, L2 hits; membership is
// what the array already says) for the last selection.  The depth keys are
// dead by then, so the peak is 2 E key registers at ps = 64, not 3 E -- that
// is what keeps CACHE = 64 free of scratch and of AGPR copies
// (profiles/surface_planes_kernel_resources.txt).  The two slant selections
// therefore do not share their group reductions; sharing them would need both
// components resident at once.  CACHE = 0 (ps > 64) re-reads both maps in
// every pass, as the parent does.
struct PlaneNodeArgs {
    double *nodes;
    uint8_t *node_valid;
    const float *depth;
    const float2 *plane;
    Grid g;
    int stride, num_nodes;
};

constexpr unsigned NO_SLANT = 0xFFFFFFFFu;

template <int CACHE>
__global__ void __launch_bounds__(256)
surf_init_nodes_planes_kernel(PlaneNodeArgs A, int G, int glog)
{
#pragma clang fp contract(off)
    Grid const g = A.g;
    int const T = g.ps * g.ps;                 // pixels of a window
    int const E = T / G;                       // per lane (<= CACHE when CACHE > 0)
    int const lane = threadIdx.x & 63;
    int const gl = lane & (G - 1);
    long long const gid = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> glog;
    bool const in_range = gid < (long long)A.num_nodes;
    int const id = in_range ? (int)gid : 0;
    int const idx = id % A.stride, idy = id / A.stride;
    bool const todo = in_range && A.node_valid[id] == 0;
    constexpr int NK = CACHE > 0 ? CACHE : 1;
    // window element e: the depth key (0: outside the image or no depth), its
    // quadrant, and the key of slant component `ch` (NO_SLANT: not in S)
    auto load = [&](int e, int ch, int *q, unsigned *skey) -> unsigned {
        int xx = 0, yy = 0;
        *q = 0;
        *skey = NO_SLANT;
        if (todo && smvs_surf::window_pixel(g, idx, idy, e, q, &xx, &yy)) {
            size_t const p = (size_t)yy * g.width + xx;
            float const d = A.depth[p];
            if (d > 0.0f) {
                float2 const s = A.plane[p];
                if (smvs_surf::slant_finite(s.x) && smvs_surf::slant_finite(s.y))
                    *skey = smvs_surf::slant_key(ch == 0 ? s.x : s.y);
                return smvs_surf::depth_key(d);
            }
        }
        return 0u;
    };
    unsigned keys[NK] = { 0u };
    unsigned skeys[NK];
    unsigned lowq[4] = { 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu };
    int count = 0, cs = 0;
    auto account = [&](unsigned key, int q, unsigned skey) {
        if (key != 0u) {
            count += 1;
            cs += skey != NO_SLANT ? 1 : 0;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (q == k)
                    lowq[k] = key < lowq[k] ? key : lowq[k];
        }
    };
    if (CACHE > 0) {
#pragma unroll
        for (int i = 0; i < NK; ++i) {
            int q = 0;
            unsigned skey = NO_SLANT;
            unsigned const key = i < E ? load(gl + G * i, 0, &q, &skey) : 0u;
            keys[i] = key;
            skeys[i] = skey;
            account(key, q, skey);
        }
    } else {
        skeys[0] = NO_SLANT;
        for (int i = 0; i < E; ++i) {
            int q = 0;
            unsigned skey = NO_SLANT;
            unsigned const key = load(gl + G * i, 0, &q, &skey);
            account(key, q, skey);
        }
    }
    // (whole groups take every branch together: the shuffles stay inside a group;
    // both counts are at most 2^20 with ps <= 1024, and at most 2^12 each where
    // they share a word)
    for (int off = G >> 1; off > 0; off >>= 1) {
        count += __shfl_xor(count, off);
        cs += __shfl_xor(cs, off);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            unsigned const o = __shfl_xor(lowq[k], off);
            lowq[k] = o < lowq[k] ? o : lowq[k];
        }
    }
    // the depth: rank selection over the positive keys, most significant bit first
    int rank = count / 2;
    unsigned prefix = 0u, mask = 0u;
    if (__any(todo && count >= 2)) {
        for (int b = 30; b >= 0; --b) {
            unsigned const bit = 1u << b;
            int zeros = 0;
            if (CACHE > 0) {
#pragma unroll
                for (int i = 0; i < NK; ++i) {
                    unsigned const key = keys[i];
                    zeros += (key != 0u && (key & mask) == prefix && (key & bit) == 0u)
                        ? 1 : 0;
                }
            } else {
                for (int i = 0; i < E; ++i) {
                    int q = 0;
                    unsigned skey;
                    unsigned const key = load(gl + G * i, 0, &q, &skey);
                    zeros += (key != 0u && (key & mask) == prefix && (key & bit) == 0u)
                        ? 1 : 0;
                }
            }
            for (int off = G >> 1; off > 0; off >>= 1)
                zeros += __shfl_xor(zeros, off);
            if (rank >= zeros) {
                rank -= zeros;
                prefix |= bit;
            }
            mask |= bit;
        }
    }
    // the slants: rank cs / 2 of the members' keys, all 32 bits
    bool const want_slants = __any(todo && count >= 2 && cs >= 1);
    unsigned sel[2] = { 0u, 0u };
    if (want_slants) {
#pragma unroll
        for (int ch = 0; ch < 2; ++ch) {
            if (CACHE > 0 && ch == 1) {
                // the second component over the first: members stay members
#pragma unroll
                for (int i = 0; i < NK; ++i)
                    if (skeys[i] != NO_SLANT) {
                        int q = 0;
                        unsigned skey = NO_SLANT;
                        (void)load(gl + G * i, 1, &q, &skey);
                        skeys[i] = skey;
                    }
            }
            int srank = cs / 2;
            unsigned sprefix = 0u, smask = 0u;
            for (int b = 31; b >= 0; --b) {
                unsigned const bit = 1u << b;
                int zeros = 0;
                if (CACHE > 0) {
#pragma unroll
                    for (int i = 0; i < NK; ++i) {
                        unsigned const key = skeys[i];
                        zeros += (key != NO_SLANT && (key & smask) == sprefix
                            && (key & bit) == 0u) ? 1 : 0;
                    }
                } else {
                    for (int i = 0; i < E; ++i) {
                        int q = 0;
                        unsigned key = NO_SLANT;
                        (void)load(gl + G * i, ch, &q, &key);
                        zeros += (key != NO_SLANT && (key & smask) == sprefix
                            && (key & bit) == 0u) ? 1 : 0;
                    }
                }
                for (int off = G >> 1; off > 0; off >>= 1)
                    zeros += __shfl_xor(zeros, off);
                if (srank >= zeros) {
                    srank -= zeros;
                    sprefix |= bit;
                }
                smask |= bit;
            }
            sel[ch] = sprefix;
        }
    }
    if (todo && gl == 0) {
        int quadrants = 4;
        double lowest[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            bool const any = lowq[k] != 0xFFFFFFFFu;
            lowest[k] = any ? (double)__uint_as_float(lowq[k]) : 0.0;
            quadrants -= any ? 0 : 1;
        }
        double node[4];
        if (smvs_surf::node_from_window_planes((double)__uint_as_float(prefix), lowest,
                quadrants, (size_t)count, (size_t)cs, smvs_surf::slant_from_key(sel[0]),
                smvs_surf::slant_from_key(sel[1]), g.ps, node)) {
            double *dst = A.nodes + 4 * (size_t)id;
            dst[0] = node[0]; dst[1] = node[1]; dst[2] = node[2]; dst[3] = node[3];
            A.node_valid[id] = 1;
        }
    }
}

void
launch_init_nodes_planes(smvs_ctx *ctx)
{
    PlaneNodeArgs A;
    A.nodes = ctx->nodes;
    A.node_valid = ctx->node_valid;
    A.depth = ctx->surf_depth;
    A.plane = reinterpret_cast<const float2 *>(ctx->surf_slant);
    A.g.width = ctx->width;
    A.g.height = ctx->height;
    A.g.scale = ctx->scale;
    A.g.ps = ctx->patchsize;
    A.g.npx = ctx->npx;
    A.g.npy = ctx->npy;
    A.g.start_x = ctx->start_x;
    A.g.start_y = ctx->start_y;
    A.stride = ctx->node_stride;
    A.num_nodes = ctx->num_nodes;
    int const ps = A.g.ps;
    if (ps < 2)
        return;   // (the window is empty, no node is initialised, surface.cc:700)
    int const T = ps * ps;
    int const G = T < 64 ? T : 64;
    int glog = 0;
    while ((1 << glog) < G)
        glog += 1;
    size_t const threads = (size_t)A.num_nodes * (size_t)G;
    dim3 const grid((unsigned)((threads + 255) / 256));
    int const E = T / G;
    if (E <= 4)
        hipLaunchKernelGGL((surf_init_nodes_planes_kernel<4>), grid, dim3(256), 0, ctx->stream,
            A, G, glog);
    else if (E <= 16)
        hipLaunchKernelGGL((surf_init_nodes_planes_kernel<16>), grid, dim3(256), 0, ctx->stream,
            A, G, glog);
    else if (E <= 64)
        hipLaunchKernelGGL((surf_init_nodes_planes_kernel<64>), grid, dim3(256), 0, ctx->stream,
            A, G, glog);
    else
        hipLaunchKernelGGL((surf_init_nodes_planes_kernel<0>), grid, dim3(256), 0, ctx->stream,
            A, G, glog);
}

} // namespace smvs_hip

using namespace smvs_hip;

extern "C" int
smvs_ctx_sgm_init_slants(smvs_ctx *ctx, const float *slant, int dm_w, int dm_h, float *out)
{
    SMVS_REQUIRE(ctx != nullptr, "null argument");
    if (slant == nullptr) {   // forget the plane
        ctx->sgm_slant_ok = false;
        return SMVS_OK;
    }
    if (!ctx->sgm_resident || ctx->sgm_lowres == nullptr) {
        set_error("smvs_ctx_sgm_init_slants: the context holds no resident SGM map "
            "(smvs_ctx_sgm_init_depth)");
        return SMVS_ERR_STATE;
    }
    SMVS_REQUIRE(dm_w == ctx->sgm_lowres_w && dm_h == ctx->sgm_lowres_h,
        "the slants do not have the size of the resident SGM map");
    SMVS_HIP_CHECK(set_device(ctx->device));
    int rc;
    size_t const n = (size_t)ctx->width * ctx->height;
    size_t const n_low = (size_t)dm_w * dm_h;
    ctx->sgm_slant_ok = false;
    if ((rc = device_grow(&ctx->sgm_slant, &ctx->sgm_slant_cap, n * 2)) != SMVS_OK)
        return rc;
    // G through the scratch buffer of the map outputs (W*H*3 floats or more
    // once it exists; grown here otherwise)
    if ((rc = device_grow(&ctx->map_scratch, &ctx->map_scratch_floats, n_low * 2)) != SMVS_OK)
        return rc;
    if ((rc = ctx_upload(ctx, ctx->map_scratch, slant, n_low * 2 * sizeof(float))) != SMVS_OK)
        return rc;
    SlantTapArgs A;
    A.lowres = ctx->sgm_lowres;
    A.slant = ctx->map_scratch;
    A.plane = reinterpret_cast<float2 *>(ctx->sgm_slant);
    A.dm_w = dm_w;
    A.dm_h = dm_h;
    A.w = ctx->width;
    A.h = ctx->height;
    hipLaunchKernelGGL(surf_slant_tap_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
        ctx->stream, A);
    SMVS_HIP_CHECK(hipGetLastError());
    ctx->sgm_slant_ok = true;
    if (out != nullptr)
        return ctx_download(ctx, out, ctx->sgm_slant, n * 2 * sizeof(float));
    return SMVS_OK;
}
