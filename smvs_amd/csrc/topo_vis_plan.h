// The launch shape of topo_visibility_kernel (topo_visibility.hip): lanes per
// (patch, neighbour), stash slots per thread and what else of the dynamic LDS
// is in use.  Host arithmetic only: no HIP, no smvs_ctx.
#pragma once

#include "topo_groups.h"

#include <algorithm>
#include <cstddef>

namespace smvs_hip {

// (three workgroups per CU -- what the kernel's registers allow -- leave
// each 53 KB of the 160)
constexpr size_t VIS_LDS_BUDGET = 52 * 1024;

struct VisLaunchShape {
    int group;               // lanes per (patch, neighbour): TopoArgs::vis_group
    int ncc_stash_slots;     // stash slots per thread
    int lds_depth_doubles;   // doubles of the staged depths (0: read from memory)
    int lds_tpl_n;           // entries of the staged interior template (0: read from memory)
    size_t dynamic_lds_bytes;   // of the launch: depths, template, stash
};

// n_max: the longest of the 32 sample templates of the patch size, tpl_n: the
// length of template 31 (interior patches).  group_override: SMVS_VIS_GROUP_<ps>
// (0: none; taken if it is 256 or a power of two up to 64), no_stash:
// SMVS_NCC_STASH=0 -- the caller reads the environment.
    // Lanes per (patch, neighbour), measured per patch size on a --no-sgm view at
    // 1920 x 1080 x 8 (profiles/r6_visibility_groups.txt; SMVS_VIS_GROUP_<ps>=<lanes>
    // is the A/B switch).  Few lanes win wherever there are enough groups to fill
    // the chip: a lane's pixels and samples are independent chains either way, and
    // the group's set-up and eleven reductions are paid once per group --
    // patch size 4 (16 pixels, 44 samples): 4 lanes 627 us, 8: 704, 16: 880;
    // patch size 8: 8 lanes 443, 16: 460, 32: 525, 64: 680; 16: 32 lanes 365, 64: 385;
    // 32: 64 lanes 310, 32: 385 (a lane's samples outgrow the stash), 256: 365;
    // 64: the workgroup 290, 64 lanes 415.
inline VisLaunchShape
vis_launch_shape(int ps, bool use_ncc, int n_max, int tpl_n, int group_override, bool no_stash)
{
    long long group = group_size(ps, VIS_WORKGROUP_FROM);
    switch (ps) {
    case 2: group = 2; break;
    case 4: group = 4; break;
    case 8: group = 8; break;
    case 16: group = 32; break;
    default: break;
    }
    int const g = group_override;
    if (g == 256 || (g >= 1 && g <= 64 && (g & (g - 1)) == 0))
        group = g;
    VisLaunchShape shape = { (int)group, 0, 0, 0, 0 };
    if (!use_ncc)
        return shape;
    int const per_lane = (int)((n_max + group - 1) / group);
    shape.ncc_stash_slots = no_stash ? 0 : std::min(NCC_STASH_MAX, std::max(0, per_lane - NCC_KEEP));
    size_t bytes = (size_t)shape.ncc_stash_slots * 3 * 256 * sizeof(float);
    size_t const depth_doubles = (size_t)(256 / group) * ((size_t)ps * ps + 4);
    if (group <= 256 && bytes + depth_doubles * 8 <= VIS_LDS_BUDGET) {
        shape.lds_depth_doubles = (int)depth_doubles;
        bytes += depth_doubles * 8;
    }
    if (bytes + (size_t)tpl_n * 8 <= VIS_LDS_BUDGET) {
        shape.lds_tpl_n = tpl_n;
        bytes += (size_t)tpl_n * 8;
    }
    shape.dynamic_lds_bytes = bytes;
    return shape;
}

} // namespace smvs_hip
