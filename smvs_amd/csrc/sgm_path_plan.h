// Which form of the SGM path aggregation (sgm_paths.hip) a run takes, what it
// needs of the workspace and which WTA kernel (sgm_wta.hip) follows.  Host
// arithmetic only: no HIP, no smvs_ctx.  The rule exists here and nowhere else.
#pragma once

namespace smvs_hip {

enum SgmPathForm {
    SGM_PATHS_WIDE,            // sgm_paths_wide_kernel: a line per wave, four planes per lane
    SGM_PATHS_PAIRS,           // sgm_paths2_kernel: two lines per wave, four planes per lane
    SGM_PATHS_LINES,           // sgm_all_paths_kernel: a line per wave, two planes per lane
    SGM_PATHS_PER_DIRECTION    // sgm_path_kernel: a launch per direction, scalar accesses
};

enum SgmWtaKernel {
    SGM_WTA_SUM_WIDE,   // sgm_sum_wta_wide_kernel: S from the path bytes, 64 lanes per pixel
    SGM_WTA_SUM,        // sgm_sum_wta_kernel: S from the path bytes, 32 lanes per pixel
    SGM_WTA_ROWS        // wta_rows_kernel: reads the u16 volume S
};

struct SgmPathPlan {
    SgmPathForm form;
    // every direction stores L - C as one byte per cell into its own volume
    // (eight of them); otherwise the paths add L into the u16 volume S
    bool delta;
    bool full;      // every lane of a line holds planes (no idle lanes to reset)
    bool zero_s;    // S is zeroed first: the paths add into it with atomics
    SgmWtaKernel wta;
    // the u16 volume S is part of the workspace: the paths write it, or the
    // caller wants it (the sum kernels then store it)
    bool needs_s(bool caller_wants_s) const { return !delta || caller_wants_s; }
};

// largest_p2: the largest penalty2 a step can use
// (SgmWorkspace::largest_penalty2).  wave_per_line: SMVS_SGM_PATHS=wave -- the
// caller reads the environment.
//
// delta: penalty2 <= 255, so L - C fits a byte; planes in fours: the u32
// accesses of the sum kernels.  Above 128 planes only the wide kernel holds a
// line in one wave; up to 128 the pairs kernel serves the byte form unless the
// caller asks for a wave per line.  Without bytes an even plane count adds u16
// pairs into S with u32 atomics; an odd one takes a launch per direction, the
// first of which writes S.
inline SgmPathPlan
sgm_path_plan(int num_steps, unsigned largest_p2, bool wave_per_line)
{
    SgmPathPlan plan;
    plan.delta = (num_steps % 4) == 0 && largest_p2 <= 255u;
    plan.full = false;
    plan.zero_s = false;
    if (num_steps > 128) {
        plan.form = SGM_PATHS_WIDE;
        plan.full = num_steps == 256;
        plan.zero_s = !plan.delta;
    } else if (plan.delta && !wave_per_line) {
        plan.form = SGM_PATHS_PAIRS;
        plan.full = num_steps == 128;
    } else if (plan.delta) {
        plan.form = SGM_PATHS_LINES;
    } else if ((num_steps % 2) == 0) {
        plan.form = SGM_PATHS_LINES;
        plan.zero_s = true;
    } else {
        plan.form = SGM_PATHS_PER_DIRECTION;
    }
    plan.wta = !plan.delta ? SGM_WTA_ROWS : (num_steps > 128 ? SGM_WTA_SUM_WIDE : SGM_WTA_SUM);
    return plan;
}

} // namespace smvs_hip
