// How many lanes work on one item of the topology kernels, and how many NCC
// samples a lane keeps.  Plain arithmetic for the kernels (topo_internal.h) and
// for the host's launch shapes (topo_vis_plan.h): no HIP needed to include it.
#pragma once

#if defined(__HIPCC__)
#define TOPO_HD __device__ __host__ __forceinline__
#else
#define TOPO_HD inline
#endif

namespace smvs_hip {

// A group of G = min(64, ps^2) consecutive lanes works on one (patch,
// neighbour) resp. one patch: the pixels / samples are dealt round-robin to
// the lanes and the group combines its partial results with xor-shuffles in a
// fixed order (deterministic).  The reference's loops are sequential; every
// quantity here is a conjunction, a maximum or a sum, so only the summation
// order differs (by rounding, far below the 0.05 / 8.0 / 0.0 thresholds the
// results are compared with).
TOPO_HD int
group_size(int ps, int whole_workgroup_from)
{
    // ps is a power of two: 1, 4, 16, 64 lanes for ps = 1, 2, 4, 8 and above.
    // From ps = whole_workgroup_from on the whole 256-thread workgroup works
    // on one item: at the coarse scales a few hundred patches of thousands of
    // pixels each are a latency chain per lane, not a throughput problem
    // (measured, 341 patches at scale 6: mse 554 -> 190 us, visibility
    // 705 -> 585 us; at ps = 16 the barriers of the workgroup-wide reductions
    // cost the visibility kernel more than the shorter chains save:
    // 840 -> 1640 us, so it switches at 64, the mse kernel at 16).
    // (Round 6: the visibility kernel takes this rule only for ps = 1, 32, 64
    // and up; in between it runs 2 / 4 / 8 / 32 lanes at ps = 2 / 4 / 8 / 16,
    // vis_launch_shape, topo_vis_plan.h.)
    int const pp = ps * ps;
    if (ps >= whole_workgroup_from)
        return 256;
    return pp >= 64 ? 64 : pp;
}
constexpr int VIS_WORKGROUP_FROM = 64;   // topo_visibility_kernel
// samples of ncc_for_patch a lane keeps in registers between the two passes;
// the following NCC_STASH_MAX live in LDS (48 KB per workgroup at most: three
// workgroups per CU, what the kernel's registers allow), any beyond are
// recomputed
constexpr int NCC_KEEP = 4;
constexpr int NCC_STASH_MAX = 16;
constexpr int MSE_WORKGROUP_FROM = 16;   // topo_mse_kernel

} // namespace smvs_hip
