// What the translation units of the topology tests share (topology.hip,
// topo_zbuffer.hip, topo_visibility.hip, topo_mse.hip, topo_cut.hip): the
// kernels' argument block, the lane-group rule and reductions, and the host
// functions that cross units.  Every kernel is launched by the unit that
// defines it.
#pragma once

#include "common.h"
#include "host/topo_math.h"
#include "topo_groups.h"

namespace smvs_hip {

using smvs_topo::NccSample;
using smvs_topo::Warp;

// three packed floats (4-byte aligned): one global_load_dwordx3
struct __attribute__((packed, aligned(4))) float3_r { float x, y, z; };

struct TopoView {
    int w, h, c;
    const float *image;   // interleaved float image (bytes / 255)
};

struct TopoArgs {
    const double *nodes;
    const uint8_t *patch_valid;
    const uint32_t *patch_vis;      // input of the mse kernel
    uint32_t *vis_out;
    double *mse_out;
    const DeviceCameras *cams;
    TopoView views[1 + SMVS_MAX_SUBS];   // [0] main, [1 + j] neighbour j
    const float2 *main_grad;
    const SubPlanes *subs;
    float *zbuf[SMVS_MAX_SUBS];     // [(h + 1)][(w + 1)] z-buffer (3 x 3 splats)
    float *zraw[SMVS_MAX_SUBS];     // same shape: nearest depth per centre cell
    // zbuf holds the 5 x 5 minimum of zraw -- the minimum of the 3 x 3 z-buffer
    // cells the visibility test compares with -- instead of the 3 x 3 one
    // (topo_dilate5_kernel; SMVS_ZBUF_WINDOW=3: the z-buffer itself, nine lookups)
    int zbuf5;
    const float *sgm_depth;         // [H][W] or nullptr
    const NccSample *ncc;           // 32 concatenated templates
    int ncc_off[33];
    int W, H, npx, npy, stride, ps, start_x, start_y, n_subs, num_patches;
    int ps_log2;       // ps = 1 << ps_log2 (Surface: patchsize = 2^scale): shifts and an
                       // exact reciprocal instead of integer and double divisions
    double inv_ps;     // 1.0 / ps
    int use_ncc;
    // cut_boundaries
    uint8_t *patch_valid_rw;
    uint8_t *node_valid_rw;
    int *deleted;               // status word
    float invproj[9];
    int num_nodes;
    // cut_boundaries: nodes with more than one missing neighbour node (the
    // state before the pass), and whether the mse kernel may skip the patches
    // that touch none of them
    uint8_t *border_node;
    int only_candidates;
    int *mse_list;      // patches topo_mse_kernel evaluates
    int *mse_count;     // status word: entries of mse_list
    // create_subview_surfaces: depth and its pixel derivatives of the surface at
    // every pixel of a valid patch, [H][W][3] doubles (topo_pixel_surface_kernel)
    double *pix;
    // SMVS_TOPO_DIVIDE=exact: every quotient by the division itself
    // (SharedDivisor; the test that both give the same bits)
    int exact_divisions;
    // SMVS_NCC_PAIRS=0: the NCC samples of a lane one after the other
    int ncc_pairs;
    // topo_visibility_kernel: lanes per (patch, neighbour) and the stash slots
    // per thread its launch reserves (vis_launch_shape)
    int vis_group, ncc_stash_slots;
    // ... and what else of its dynamic LDS is in use: doubles of the staged
    // depths (0: read from memory), entries of the staged interior template
    int lds_depth_doubles, lds_tpl_n;
    // topo_mse_kernel at patch sizes 32 / 64: chunks of 256 pixels per patch,
    // their partial sums [item][chunk][2] and arrival counters [item] (zero
    // between launches)
    int mse_chunks;
    double *mse_parts;
    int *mse_arrived;
};

__device__ __forceinline__ void
load_patch_nodes(TopoArgs const &A, int p, double n16[16])
{
    int const ix = p % A.npx, iy = p / A.npx;
    int const n00 = iy * A.stride + ix;
    int const ids[4] = { n00, n00 + 1, n00 + A.stride, n00 + A.stride + 1 };
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int k = 0; k < 4; ++k)
            n16[4 * n + k] = A.nodes[4 * (size_t)ids[n] + k];
}

// min over floats of any sign with integer atomics
__device__ __forceinline__ void
atomic_min_float(float *addr, float v)
{
    if (v >= 0.0f)
        atomicMin(reinterpret_cast<int *>(addr), __float_as_int(v));
    else
        atomicMax(reinterpret_cast<unsigned int *>(addr), __float_as_uint(v));
}

// Reductions over a lane group (the patch-MSE kernel's; the visibility
// kernel's are vis_lanes_reduce below).  G <= 64: xor-shuffles inside the wave.
// G == 256: the workgroup is the group -- per-wave results meet in LDS (every
// thread of the workgroup must call; `red` holds 4 doubles).
template <typename T>
__device__ __forceinline__ T
group_sum(T v, int G, double *red)
{
    for (int off = (G < 64 ? G : 64) >> 1; off > 0; off >>= 1)
        v += __shfl_xor(v, off);
    if (G > 64) {
        __syncthreads();   // (the previous reduction's readers are done)
        if ((threadIdx.x & 63) == 0)
            red[threadIdx.x >> 6] = (double)v;
        __syncthreads();
        v = (T)(((red[0] + red[1]) + red[2]) + red[3]);
    }
    return v;
}

__device__ __forceinline__ bool
group_all(bool ok, int G, int lane, double *red)
{
    unsigned long long const b = __ballot(ok);
    if (G > 64)
        return __syncthreads_and(b == ~0ull) != 0;
    (void)red;
    unsigned long long const gmask = G >= 64 ? ~0ull
        : (((1ull << G) - 1ull) << ((lane / G) * G));
    return (b & gmask) == gmask;
}

// The end of both candidate kernels: patch p of every `alive` thread is
// appended to A.mse_list (every thread of the workgroup must call).
__device__ __forceinline__ void
append_listed(TopoArgs const &A, bool alive, int p)
{
    // one atomic per workgroup: the list's end is one word for the whole grid
    __shared__ int wave_count[4];
    __shared__ int block_base;
    unsigned long long const mask = __ballot(alive);
    int const lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0)
        wave_count[wave] = __popcll(mask);
    __syncthreads();
    if (threadIdx.x == 0) {
        int const total = wave_count[0] + wave_count[1] + wave_count[2] + wave_count[3];
        block_base = total > 0 ? atomicAdd(A.mse_count, total) : 0;
    }
    __syncthreads();
    if (alive) {
        int at = block_base + __popcll(mask & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; ++w)
            at += wave_count[w];
        A.mse_list[at] = p;
    }
}

// ---- host functions that cross translation units ----
// The argument block from the context's state (topology.hip); `who` names the
// entry point in error messages.
int fill_args(smvs_ctx *ctx, TopoArgs *A, const char *who);
// Every neighbour's z-buffer of the current surface and of A.sgm_depth
// (topo_zbuffer.hip).  Enqueues only.
void launch_zbuffers(smvs_ctx *ctx, TopoArgs const &A);
// The surface at every pixel, then the visibility masks (topo_visibility.hip);
// chooses the launch shape and stores it in *A.
int launch_visibility(smvs_ctx *ctx, TopoArgs *A);
// Buffers and arguments of the patch-MSE kernels; the candidate list and the
// errors of its entries; the errors of a list that is on the stream
// (topo_mse.hip)
int prepare_patch_mse(smvs_ctx *ctx, TopoArgs *A, const char *who);
int launch_patch_mse(smvs_ctx *ctx, TopoArgs const &A, bool count_is_zero);
int launch_patch_mse_listed(smvs_ctx *ctx, TopoArgs const &A);

} // namespace smvs_hip
