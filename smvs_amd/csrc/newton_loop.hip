// The host driver of the Newton loop (smvs_gn_run_loop, reference:
// lib/depth_optimizer.cc:214-303): the launches of newton_step.h one step at
// a time or launch-ahead, and the steps' result words.  No kernels.
#include "newton_step.h"

#include <chrono>

using namespace smvs_hip;

// State of one smvs_gn_run_loop call
struct LoopState {
    int num_initial = 0;
    int num_active = 0;
    int newton_step = 0;
    int known_live = -1;   // length of the live-patch list once read back
    bool ended = false;    // a break of depth_optimizer.cc:267-268 / :284-288
    int begin_seq = 0;     // tag of the loop-begin words while they are unread
    double last_update = -1.0;   // full optimisation: mean shift of the newest step
};

static bool
loop_goes_on(const smvs_gn_loop_params *prm, LoopState const &L)
{
    // depth_optimizer.cc:219-220
    return !L.ended && L.newton_step < prm->max_newton_steps
        && L.num_active > L.num_initial / 20;
}

// Spins on a result slot until finish_step_kernel has published `seq` there:
// the next launches follow the end of the step within microseconds (no stream
// query, no copies).
static int
wait_step_words(smvs_ctx *ctx, int seq, const int **slot_out)
{
    const int *words = step_slot(ctx, seq);
    auto const t_start = std::chrono::steady_clock::now();
    long spins = 0;
    while (__atomic_load_n(&words[STEP_SEQ], __ATOMIC_ACQUIRE) != seq) {
        __builtin_ia32_pause();
        if ((++spins & 0xFFFF) == 0) {
            hipError_t const q = hipStreamQuery(ctx->stream);
            if (q != hipSuccess && q != hipErrorNotReady)
                SMVS_HIP_CHECK(q);
            if (q == hipSuccess
                && __atomic_load_n(&words[STEP_SEQ], __ATOMIC_ACQUIRE) != seq) {
                set_error("smvs_gn_run_loop: the step ended without "
                    "publishing its result");
                return SMVS_ERR_STATE;
            }
            if (std::chrono::steady_clock::now() - t_start
                > std::chrono::seconds(60)) {
                set_error("smvs_gn_run_loop: timed out waiting for the device");
                return SMVS_ERR_STATE;
            }
        }
    }
    *slot_out = words;
    return SMVS_OK;
}

// The counts loop_begin_launch published: the initial active set and the
// length of the first live list.
static int
read_loop_begin(smvs_ctx *ctx, LoopState &L)
{
    const int *words = nullptr;
    int const rc = wait_step_words(ctx, L.begin_seq, &words);
    if (rc != SMVS_OK)
        return rc;
    L.num_initial = L.num_active = words[STEP_NUM_ACTIVE];
    L.known_live = words[STEP_NEXT_LIVE];
    L.begin_seq = 0;
    return SMVS_OK;
}

// The bookkeeping of depth_optimizer.cc:267-303 on a step's result words.
static void
account_step(const smvs_gn_loop_params *prm, smvs_gn_loop_stats *stats,
    LoopState &L, const int *words, int cg_iterations)
{
    L.newton_step += 1;
    stats->linear_iterations += cg_iterations;
    stats->active_patch_steps += words[STEP_ACTIVE_PATCHES];
    L.known_live = words[STEP_NEXT_LIVE];
    if (words[STEP_NAN] != 0) {
        stats->nan_break = 1;
        L.ended = true;
        return;
    }
    if (prm->full_optimization) {
        // depth_optimizer.cc:277-288: sum_diff / size; with no reprojection
        // term at all this is 0 / 0 = NaN, the comparison is false and the
        // loop goes on to its step limit like the reference
        const double *sc = reinterpret_cast<const double *>(words + STEP_SCALARS);
        L.last_update = sc[0] / sc[1];
        if (L.last_update < prm->full_opt_threshold)
            L.ended = true;
        return;
    }
    L.num_active = words[STEP_NUM_ACTIVE];
}

static int
next_step_seq(smvs_ctx *ctx)
{
    ctx->step_seq = (ctx->step_seq % 0x3FFFFFFF) + 1;
    return ctx->step_seq;
}

// SMVS_LOOP_TEST (tests/test_gpu_parity.py, tools/cg_trace.py): "undersize"
// sizes every launch-ahead step for half the list, "solver" makes the second
// solve of a loop report that it gave up, "unpipelined" runs the fused steps
// one at a time (the host waits for each solve: what SMVS_CG_TRACE needs),
// "wide" uses the end-of-step kernel's counters for surfaces of 2^24 nodes and
// more on any surface.
LoopTest
smvs_hip::loop_test_mode(void)
{
    static LoopTest const mode = [] {
        const char *e = std::getenv("SMVS_LOOP_TEST");
        if (e == nullptr)
            return LOOP_TEST_NONE;
        return std::strcmp(e, "undersize") == 0 ? LOOP_TEST_UNDERSIZE
            : std::strcmp(e, "solver") == 0 ? LOOP_TEST_SOLVER
            : std::strcmp(e, "unpipelined") == 0 ? LOOP_TEST_UNPIPELINED
            : std::strcmp(e, "wide") == 0 ? LOOP_TEST_WIDE : LOOP_TEST_NONE;
    }();
    return mode;
}

// One Newton step, the host waits for its result before it launches the next
// one: with the assembly kernel and the streaming solver, or (test mode
// "unpipelined") with the fused resident solver.
static int
run_step_streaming(smvs_ctx *ctx, const smvs_gn_loop_params *prm,
    smvs_gn_loop_stats *stats, LoopState &L)
{
    int rc;
    bool const fused = loop_test_mode() == LOOP_TEST_UNPIPELINED
        && cg_resident_applies(ctx, prm->cg_max_iterations);
    if ((rc = gn_construct_launch(ctx, prm->regularization,
            prm->light_surf_regularization, prm->use_lighting != 0,
            L.known_live, fused)) != SMVS_OK)
        return rc;
    int iters = 0, info = 0;
    bool solved = false;
    if (fused && (rc = cg_resident_solve(ctx, prm->cg_max_iterations, -1.0,
            prm->cg_q_tolerance, &iters, &info, &solved, true)) != SMVS_OK)
        return rc;
    if (!solved) {
        if (fused && (rc = gn_assemble_launch(ctx)) != SMVS_OK)
            return rc;
        if ((rc = cg_solve_launch(ctx, prm->cg_max_iterations, -1.0,
                prm->cg_q_tolerance, &iters, &info)) != SMVS_OK)
            return rc;
    }
    int const seq = next_step_seq(ctx);
    if ((rc = step_end_launch(ctx, prm->active_threshold, prm->full_optimization,
            StepEnd{ seq, L.known_live, false, 0.0 })) != SMVS_OK)
        return rc;
    const int *words = nullptr;
    if ((rc = wait_step_words(ctx, seq, &words)) != SMVS_OK)
        return rc;
    account_step(prm, stats, L, words, iters);
    return SMVS_OK;
}

// The Newton loop with the fused resident solver, launch-ahead: step k + 1 is
// enqueued before the result of step k is known, so the GPU never waits for
// the host between steps.  The kernels size themselves from the device-side
// list length; finish_step_kernel evaluates the loop condition into
// status[I_STOP], and a step enqueued behind the end of the loop does nothing
// but report that it was skipped.  Returns with L.ended set, or -- when the
// solver gave up -- with the context's resident solver disabled and L at the
// last completed step (the caller goes on with run_step_streaming).
static int
run_steps_pipelined(smvs_ctx *ctx, const smvs_gn_loop_params *prm,
    smvs_gn_loop_stats *stats, LoopState &L)
{
    // the loop's share of the device's CUs (tile_budget.h): the
    // barrier kernels running side by side never ask for more workgroups than
    // the device can keep resident together
    ScopedTileBudget guard(cg_resident_budget(ctx->device), cg_resident_tiles(ctx));
    static_assert(I_STEP_ABORT == I_STOP + 1, "cleared together");
    LoopTest const test_mode = loop_test_mode();
    int rc;
    int seqs[2] = { 0, 0 };      // tags of the steps in flight, oldest first
    int in_flight = 0;
    int enqueued = L.newton_step;   // steps enqueued so far (absolute number)
    auto enqueue = [&]() -> int {
        StepEnd E;
        E.seq = next_step_seq(ctx);
        E.ahead = true;
        // The launches are sized for the newest list length the host has
        // seen -- one step old when the launch is ahead -- plus some slack
        // (the surplus workgroups leave at once; a list that still came out
        // longer makes the step abandon itself, below), for every patch
        // before the first count has come back.  Multiples of 32 patches:
        // the patch kernel's 8 bands of 4-patch workgroups.
        long long want = ctx->num_patches;
        if (L.known_live >= 0 && L.known_live + L.known_live / 16 + 64 < want)
            want = L.known_live + L.known_live / 16 + 64;
        // (test hooks, see loop_test_mode)
        if (test_mode == LOOP_TEST_UNDERSIZE && in_flight >= 1 && L.known_live >= 0)
            want = L.known_live / 2;
        E.live = (int)((want + 31) / 32 * 32);
        E.full_opt_threshold = prm->full_opt_threshold;
        int r = gn_construct_launch(ctx, prm->regularization,
            prm->light_surf_regularization, prm->use_lighting != 0,
            E.live, true, true);
        if (r == SMVS_OK)
            r = cg_resident_enqueue(ctx, prm->cg_max_iterations,
                prm->cg_q_tolerance, test_mode == LOOP_TEST_SOLVER && enqueued == 1);
        if (r == SMVS_OK)
            r = step_end_launch(ctx, prm->active_threshold,
                prm->full_optimization, E);
        if (r == SMVS_OK) {
            seqs[in_flight++] = E.seq;
            enqueued += 1;
        }
        return r;
    };
    // every enqueued step is waited for before this function returns (the
    // result slots and the stop words are then quiet)
    auto drain = [&]() -> int {
        while (in_flight > 0) {
            const int *words = nullptr;
            int const q = wait_step_words(ctx, seqs[0], &words);
            seqs[0] = seqs[1];
            in_flight -= 1;
            if (q != SMVS_OK)
                return q;
        }
        return SMVS_OK;
    };
    // An error exit must not release the device's barrier-kernel mutex while
    // launches of this loop may still be in flight: wait for the stream (the
    // result words may never come, so no drain()).
    auto fail = [&](int r) -> int {
        (void)hipStreamSynchronize(ctx->stream);
        return r;
    };
    if ((rc = enqueue()) != SMVS_OK)
        return fail(rc);
    // A step enqueued behind the end of the loop costs four empty launches
    // (~20 us); a step that was not enqueued ahead costs the host's turn-around
    // (~25 us) once its predecessor has ended.  So the next step is enqueued
    // ahead only while the loop is likely to go on: the active set (one step
    // old) is still well above the level at which the loop stops, the mean
    // shift of full optimisation well above its threshold, and -- before the
    // first result -- the previous loop on this context ran that far.
    auto likely_to_go_on = [&]() -> bool {
        if (test_mode == LOOP_TEST_UNDERSIZE)
            return true;
        if (L.newton_step == 0)
            return ctx->last_loop_steps > enqueued;
        if (prm->full_optimization)
            return !(L.last_update < 4.0 * prm->full_opt_threshold);
        return L.num_active / 4 > L.num_initial / 20;
    };
    for (;;) {
        if (enqueued < prm->max_newton_steps
            && (in_flight == 0 || (in_flight < 2 && likely_to_go_on())))
            if ((rc = enqueue()) != SMVS_OK)
                return fail(rc);
        if (L.begin_seq != 0) {
            // (published long before the first step ends)
            if ((rc = read_loop_begin(ctx, L)) != SMVS_OK)
                return fail(rc);
            if (!loop_goes_on(prm, L)) {
                // no active node: the steps in flight report themselves skipped
                L.ended = true;
                return drain();
            }
        }
        const int *words = nullptr;
        if ((rc = wait_step_words(ctx, seqs[0], &words)) != SMVS_OK)
            return fail(rc);
        seqs[0] = seqs[1];
        in_flight -= 1;
        int const gate = words[STEP_GATE];
        if (gate == GATE_ABANDONED + ABORT_SOLVER || gate == GATE_ABANDONED + ABORT_GRID) {
            // this step and the one behind it did nothing
            bool const solver = gate == GATE_ABANDONED + ABORT_SOLVER;
            if ((rc = drain()) != SMVS_OK)
                return fail(rc);
            SMVS_HIP_CHECK(hipMemsetAsync(ctx->status + I_STOP, 0,
                2 * sizeof(int), ctx->stream));
            enqueued = L.newton_step;
            if (solver) {
                // its workgroups were not all resident: never try again on
                // this context, the caller goes on with the streaming solver
                return cg_resident_gave_up(ctx);
            }
            // the live list outgrew the launch: again, sized for the list
            // length that has come back in the meantime
            if ((rc = enqueue()) != SMVS_OK)
                return fail(rc);
            continue;
        }
        if (gate != GATE_RAN) {
            set_error("smvs_gn_run_loop: a step was skipped before the loop ended");
            return fail(SMVS_ERR_STATE);
        }
        ctx->last_cg_iterations = words[STEP_CG_ITERS];
        account_step(prm, stats, L, words, words[STEP_CG_ITERS]);
        if (!L.ended && !(L.num_active > L.num_initial / 20))
            L.ended = true;
        if (L.ended != (words[STEP_LOOP_ENDS] != 0)) {
            set_error("smvs_gn_run_loop: host and device disagree on the end "
                "of the loop");
            return fail(SMVS_ERR_STATE);
        }
        if (L.ended || L.newton_step >= prm->max_newton_steps)
            break;
    }
    // (a step enqueued behind the end reports itself skipped)
    rc = drain();
    L.ended = true;
    ctx->last_loop_steps = L.newton_step;
    return rc;
}

extern "C" int
smvs_gn_run_loop(smvs_ctx *ctx, const smvs_gn_loop_params *prm,
    smvs_gn_loop_stats *stats)
{
    SMVS_REQUIRE(ctx && prm && stats, "null argument");
    if (!ctx->has_surface || !ctx->has_cameras) {
        set_error("smvs_gn_run_loop: no surface / cameras");
        return SMVS_ERR_STATE;
    }
    if (prm->use_lighting && !ctx->has_shading) {
        set_error("smvs_gn_run_loop: lighting requested without shading planes");
        return SMVS_ERR_STATE;
    }
    SMVS_REQUIRE(prm->max_newton_steps >= 0, "max_newton_steps is negative");
    SMVS_REQUIRE(prm->active_threshold >= 0.0 && prm->full_opt_threshold >= 0.0
        && prm->cg_q_tolerance >= 0.0, "negative threshold");
    // (the iteration number travels in the low 16 bits of the solvers' tags,
    // as in cg_solve_launch; the neighbour planes are checked by
    // gn_construct_launch, shared with the stand-alone entry point)
    SMVS_REQUIRE(prm->cg_max_iterations >= 0 && prm->cg_max_iterations <= 0xFFFF,
        "cg_max_iterations out of range [0, 65535]");
    SMVS_HIP_CHECK(set_device(ctx->device));
    memset(stats, 0, sizeof(*stats));
    int rc;
    if (prm->use_lighting)
        SMVS_HIP_CHECK(hipMemcpyAsync(ctx->lighting, prm->lighting,
            16 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));

    LoopState L;
    if (prm->max_newton_steps == 0) {
        // nothing to run: only the count of the active set is reported
        int num_initial = 0;
        if (prm->reset_active
            && (rc = smvs_ctx_set_active(ctx, nullptr)) != SMVS_OK)
            return rc;
        if ((rc = smvs_get_active(ctx, nullptr, &num_initial)) != SMVS_OK)
            return rc;
        L.num_initial = L.num_active = num_initial;
    } else {
        // the start of the loop happens on the device (no round trip before
        // the first step): active set, its size, the first live list
        L.begin_seq = next_step_seq(ctx);
        if ((rc = loop_begin_launch(ctx, prm->reset_active != 0, L.begin_seq))
                != SMVS_OK)
            return rc;
    }
    while (L.begin_seq != 0 || loop_goes_on(prm, L)) {
        // With the resident solver the assembly happens inside the solve (H,
        // g and P never travel through HBM) and the steps are enqueued ahead
        // of their predecessors' results; if it cannot run -- or gives up
        // because its workgroups were not all resident -- the assembly kernel
        // and the streaming solver take over, one step at a time.
        if (loop_test_mode() != LOOP_TEST_UNPIPELINED
            && cg_resident_applies(ctx, prm->cg_max_iterations)) {
            if ((rc = run_steps_pipelined(ctx, prm, stats, L)) != SMVS_OK)
                return rc;
            continue;
        }
        if (L.begin_seq != 0) {
            if ((rc = read_loop_begin(ctx, L)) != SMVS_OK)
                return rc;
            continue;
        }
        if ((rc = run_step_streaming(ctx, prm, stats, L)) != SMVS_OK)
            return rc;
    }
    stats->newton_steps = L.newton_step;
    stats->final_active_nodes = L.num_active;
    return SMVS_OK;
}
