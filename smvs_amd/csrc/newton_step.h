// The Newton step between its translation units: its result words, the abort
// reasons, the test hook, the launches newton_loop.hip strings together.
#pragma once

#include "common.h"

namespace smvs_hip {

// Result words of a Newton step in its pinned slot (step_slot), published by
// finish_step_kernel (reactivate.hip).
enum {
    STEP_SEQ = 0,          // the sequence tag, stored last
    STEP_NUM_ACTIVE,       // active nodes
    STEP_NAN,              // delta[0] was NaN: nothing was updated
    STEP_ACTIVE_PATCHES,   // active patches of the step
    STEP_NEXT_LIVE,        // length of the next live-patch list
    STEP_GATE,             // GATE_*
    STEP_CG_ITERS,         // CG iterations
    STEP_LOOP_ENDS,        // the loop ends after this step
    STEP_SCALARS           // two doubles: sum of shifts, number of terms
};
constexpr int STEP_SLOTS = 4;        // steps whose result words can coexist
constexpr int STEP_SLOT_INTS = 16;   // one 64-byte line per slot
inline int *
step_slot(const smvs_ctx *ctx, int seq)   // where the step tagged `seq` publishes
{
    return ctx->step_words + (seq & (STEP_SLOTS - 1)) * STEP_SLOT_INTS;
}

// reasons in status[I_STEP_ABORT]
constexpr int ABORT_SOLVER = 1;   // the resident solver gave up (workgroups not co-resident)
constexpr int ABORT_GRID = 2;     // a launch was sized for a shorter live list
// STEP_GATE of a step enqueued ahead.  (Sums of constants, no function: behind
// a call the compiler ordered finish_step_kernel's first loads differently.)
constexpr int GATE_RAN = 0;
constexpr int GATE_SKIPPED = 1;     // the loop had ended
constexpr int GATE_ABANDONED = 1;   // + the ABORT_* reason

// SMVS_LOOP_TEST (newton_loop.hip)
enum LoopTest { LOOP_TEST_NONE = 0, LOOP_TEST_UNDERSIZE, LOOP_TEST_SOLVER,
    LOOP_TEST_UNPIPELINED, LOOP_TEST_WIDE };
LoopTest loop_test_mode(void);

struct StepEnd {   // the end of a step inside the Newton loop
    int seq;      // sequence tag finish_step_kernel publishes (never 0)
    int live;     // list length the launches are sized for; negative: no list, every patch
    bool ahead;   // launch-ahead: sized and enqueued before the previous step's result is
                  // known; the kernels read the list length and the stop words on the device
    double full_opt_threshold;   // read only when `ahead`
};

// Stand-alone update: re-activation over every patch, apply_update_kernel.
int reactivate_launch(smvs_ctx *ctx, double threshold, int full_optimization);
// The loop's: re-activation over the live list, then finish_step_kernel (node
// update, next live list, the result words under E.seq).
int step_end_launch(smvs_ctx *ctx, double threshold, int full_optimization,
    StepEnd const &E);
// Start of a Newton loop (depth_optimizer.cc:214-220) without a host round
// trip: optionally active := valid nodes, count the active set into
// status[I_NUM_INITIAL], build the first live-patch list, clear the stop /
// abort words, publish the counts under `seq`.
int loop_begin_launch(smvs_ctx *ctx, bool reset_active, int seq);
// known_live: entries of the live-patch list the previous end of step of the
// same Newton loop built (its count read back by the host), or -1 to build
// the list here.
// skip_assembly: leave the per-patch systems unassembled (the resident solver
// gathers them itself, cg_resident_solve(..., fused = true)).
int gn_construct_launch(smvs_ctx *ctx, double reg, double light_reg,
    bool use_lighting, int known_live = -1, bool skip_assembly = false,
    bool check_stop = false);
int gn_assemble_launch(smvs_ctx *ctx);
int live_patch_list_launch(smvs_ctx *ctx);
int cg_solve_launch(smvs_ctx *ctx, int max_iterations, double error_tolerance,
    double q_tolerance, int *num_iterations, int *info);
// fused: assemble H, g, P from the per-patch systems inside the kernel (the
// caller has NOT run the assembly kernel); *ran = false means nothing was done.
int cg_resident_solve(smvs_ctx *ctx, int max_iterations, double error_tolerance,
    double q_tolerance, int *num_iterations, int *info, bool *ran,
    bool fused = false);
bool cg_resident_applies(smvs_ctx *ctx, int max_iterations);
// the tile budget (tile_budget.h) of the GPU behind a logical device
DeviceTileBudget &cg_resident_budget(int device);
// workgroups (= tiles = CUs) the resident solver launches for this context's
// grid; 0 when it does not apply
int cg_resident_tiles(smvs_ctx *ctx);
int cg_resident_enqueue(smvs_ctx *ctx, int max_iterations, double q_tolerance,
    bool test_give_up = false);
int cg_resident_gave_up(smvs_ctx *ctx);   // a resident solve failed: what runs from now on

} // namespace smvs_hip
