// C ABI of the host mirror (host_capi.h): the error slot, DepthOptimizer on one
// view and on a ViewQueue, its embeddings and recorded loops, and the
// reference's own Newton-step classes.
#include "capi_internal.h"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>

#include "conjugate_gradient.h"
#include "depth_optimizer.h"
#include "gauss_newton_step.h"
#include "view_queue.h"

using namespace smvs_amd;
using namespace smvs_amd::capi;

thread_local std::string smvs_amd::capi::g_host_error;

extern "C" const char *
smvs_host_last_error(void)
{
    return g_host_error.c_str();
}

// the main view's embeddings after this thread's last smvs_host_optimize
static std::map<std::string, FloatImage::Ptr>&
last_embeddings(void)
{
    static thread_local std::map<std::string, FloatImage::Ptr> m;
    return m;
}

static DepthOptimizer::Options
optimizer_options(smvs_host_options const& o)
{
    DepthOptimizer::Options opts;
    opts.regularization = o.regularization;
    opts.light_surf_regularization = o.light_surf_regularization;
    opts.num_iterations = o.num_iterations;
    opts.min_scale = o.min_scale;
    opts.use_shading = o.use_shading != 0;
    opts.use_sgm = o.use_sgm != 0;
    opts.full_optimization = o.full_optimization != 0;
    opts.device = o.device;
    opts.solver = o.solver;
    return opts;
}

static void
fill_log(DepthOptimizer const& optimizer, smvs_host_log *log)
{
    log->count = 0;
    for (auto const& e : optimizer.get_log()) {
        if (log->count >= SMVS_HOST_LOG_MAX)
            break;
        int const i = log->count++;
        log->scale[i] = e.scale;
        log->iter[i] = e.iter;
        log->newton_steps[i] = e.newton_steps;
        log->valid_patches[i] = e.valid_patches;
        log->cg_iterations[i] = e.cg_iterations;
        log->active_patch_steps[i] = e.active_patch_steps;
        log->loop_seconds[i] = e.loop_seconds;
    }
    log->has_lighting = optimizer.has_lighting() ? 1 : 0;
    std::copy(optimizer.get_lighting(), optimizer.get_lighting() + 16,
        log->lighting);
}

// depth_out / normals_out (either may be NULL) of a view of npix pixels
static void
copy_maps(DepthOptimizer& optimizer, std::size_t npix, float *depth_out, float *normals_out)
{
    if (depth_out != nullptr)
        std::memcpy(depth_out, optimizer.get_depth()->begin(), sizeof(float) * npix);
    if (normals_out != nullptr)
        std::memcpy(normals_out, optimizer.get_normals()->begin(), sizeof(float) * 3 * npix);
}

extern "C" int
smvs_host_optimize(const smvs_host_view *main_in, const smvs_host_view *subs_in,
    int n_subs, const smvs_host_bundle *bundle_in, const float *sgm_depth,
    int sgm_w, int sgm_h, float *sgm_roundtrip, const smvs_host_options *o,
    float *depth_out, float *normals_out, smvs_host_log *log)
{
    return smvs_host_optimize_planes(main_in, subs_in, n_subs, bundle_in, sgm_depth, sgm_w,
        sgm_h, sgm_roundtrip, nullptr, 0, 0, 0, o, 0u, depth_out, normals_out, log);
}

extern "C" int
smvs_host_optimize_flags(const smvs_host_view *main_in, const smvs_host_view *subs_in,
    int n_subs, const smvs_host_bundle *bundle_in, const float *sgm_depth,
    int sgm_w, int sgm_h, float *sgm_roundtrip, const smvs_host_options *o,
    unsigned flags, float *depth_out, float *normals_out, smvs_host_log *log)
{
    // (this entry knows its one bit; the newer ones are smvs_host_optimize_planes')
    int const status = guarded([&] {
        require((flags & ~(unsigned)SMVS_HOST_OPTIMIZE_DEVICE_SHADING_PREP) == 0u,
            "smvs_host_optimize_flags: unknown flag");
    });
    return status != 0 ? status : smvs_host_optimize_planes(main_in, subs_in, n_subs, bundle_in, sgm_depth, sgm_w,
        sgm_h, sgm_roundtrip, nullptr, 0, 0, 0, o, flags, depth_out, normals_out, log);
}

extern "C" int
smvs_host_optimize_planes(const smvs_host_view *main_in, const smvs_host_view *subs_in,
    int n_subs, const smvs_host_bundle *bundle_in, const float *sgm_depth,
    int sgm_w, int sgm_h, float *sgm_roundtrip, const float *sgm_slant, int slant_w,
    int slant_h, int slant_channels, const smvs_host_options *o,
    unsigned flags, float *depth_out, float *normals_out, smvs_host_log *log)
{
    return guarded([&] {
        require((flags & ~(unsigned)(SMVS_HOST_OPTIMIZE_DEVICE_SHADING_PREP
            | SMVS_HOST_OPTIMIZE_INIT_SLANTS)) == 0u, "smvs_host_optimize_planes: unknown flag");
        require(sgm_slant == nullptr || (slant_w >= 1 && slant_h >= 1 && slant_channels >= 1),
            "smvs_host_optimize_planes: bad slant map");
        // (the previous call's embeddings go back to the page-locked pool BEFORE
        // this call asks it for its maps: kept until the next call's end, the 33 MB
        // of a 1920 x 1080 depth + normal pair were allocated afresh every time --
        // 6.4 instead of 0.7 ms for `depth + normal maps`)
        last_embeddings().clear();
        StereoView::Ptr main_view = make_view(*main_in, o->use_shading != 0,
            o->gamma_correction != 0);
        std::vector<StereoView::Ptr> subs = make_views(subs_in, n_subs);
        Bundle::Ptr bundle = make_bundle(bundle_in);
        if (sgm_depth != nullptr) {
            main_view->write_depth_to_view_deferred(float_image_from(sgm_depth, sgm_w, sgm_h,
                1), "smvs-sgm");
            if (sgm_roundtrip != nullptr)
                std::memcpy(sgm_roundtrip, main_view->get_sgm_depth()->begin(),
                    sizeof(float) * sgm_w * sgm_h);
        }
        if (sgm_slant != nullptr)
            main_view->write_image_to_view(float_image_from(sgm_slant, slant_w, slant_h,
                slant_channels), "smvs-sgm-slant");
        DepthOptimizer::Options opts = optimizer_options(*o);
        opts.device_shading_prep = (flags & SMVS_HOST_OPTIMIZE_DEVICE_SHADING_PREP) != 0u;
        opts.init_slants = (flags & SMVS_HOST_OPTIMIZE_INIT_SLANTS) != 0u;
        // (the test harness sets Options::debug_lvl through the environment:
        // smvs_host_options is mirrored field for field by smvs_amd/host.py)
        if (const char *lvl = std::getenv("SMVS_DEBUG_LVL"))
            opts.debug_lvl = std::atoi(lvl);
        DepthOptimizer optimizer(main_view, subs, bundle, opts);
        optimizer.optimize();
        copy_maps(optimizer, (std::size_t)main_in->width * main_in->height, depth_out,
            normals_out);
        if (log != nullptr)
            fill_log(optimizer, log);
        last_embeddings() = main_view->get_embeddings();
    });
}

extern "C" int
smvs_host_shading_planes(const uint8_t *bytes, int width, int height, int channels,
    int gamma, float *shading_out, float *grad_out)
{
    return guarded([&] {
        require(bytes != nullptr && width >= 1 && height >= 1 && channels >= 1,
            "smvs_host_shading_planes: bad argument");
        StereoView::Ptr view = StereoView::create(0, byte_image_from(bytes, width, height,
            channels), CameraInfo(), true, gamma != 0);
        std::size_t const npix = (std::size_t)width * height;
        if (shading_out != nullptr)
            std::memcpy(shading_out, view->get_shading_image()->begin(),
                sizeof(float) * npix);
        if (grad_out != nullptr)
            std::memcpy(grad_out, view->get_shading_gradients()->begin(),
                sizeof(float) * 2 * npix);
    });
}

extern "C" int
smvs_host_gamma_inv_srgb_lut(float *out256)
{
    return guarded([&] {
        require(out256 != nullptr, "smvs_host_gamma_inv_srgb_lut: bad argument");
        imgtools::gamma_inv_srgb_lut(out256);
    });
}

extern "C" int
smvs_host_embedding_names(char *names_out, int cap)
{
    std::string all;
    for (auto const& kv : last_embeddings())
        all += kv.first + "\n";
    if (names_out != nullptr && cap > 0) {
        std::size_t const n = std::min(all.size(), (std::size_t)cap - 1);
        std::memcpy(names_out, all.data(), n);
        names_out[n] = 0;
    }
    return (int)last_embeddings().size();
}

extern "C" int
smvs_host_embedding(const char *name, float *out, long long cap_floats, int *whc)
{
    auto it = last_embeddings().find(name ? name : "");
    if (it == last_embeddings().end() || it->second == nullptr)
        return -1;
    FloatImage::Ptr img = it->second;
    long long const n = (long long)img->get_pixel_amount() * img->channels();
    if (whc != nullptr) {
        whc[0] = img->width();
        whc[1] = img->height();
        whc[2] = img->channels();
    }
    if (out == nullptr || cap_floats < n)
        return (int)n;
    std::memcpy(out, img->begin(), sizeof(float) * (std::size_t)n);
    return 0;
}

extern "C" int
smvs_host_release_recorded_loops(int destroy)
{
    auto& loops = recorded_loops();
    int const n = (int)loops.size();
    if (destroy)
        for (auto& l : loops)
            (void)smvs_ctx_destroy(l.ctx);
    loops.clear();
    return n;
}

extern "C" int
smvs_host_record_loops(int on)
{
    if (on)
        (void)smvs_host_release_recorded_loops(1);
    recording_loops() = on != 0;
    return 0;
}

extern "C" int
smvs_host_recorded_loops(void **ctxs, void *params, int *scales, int *iters, int cap)
{
    auto const& loops = recorded_loops();
    smvs_gn_loop_params *prm = static_cast<smvs_gn_loop_params *>(params);
    for (int i = 0; i < (int)loops.size() && i < cap; ++i) {
        if (ctxs != nullptr)
            ctxs[i] = loops[i].ctx;
        if (prm != nullptr)
            prm[i] = loops[i].params;
        if (scales != nullptr)
            scales[i] = loops[i].scale;
        if (iters != nullptr)
            iters[i] = loops[i].iter;
    }
    return (int)loops.size();
}

extern "C" int
smvs_host_optimize_views(const smvs_host_view *mains, const smvs_host_view *subs_in,
    int n_jobs, int n_subs, const smvs_host_bundle *bundle_in,
    const smvs_host_options *o, int sgm_scale, int first_device, int num_devices,
    int views_in_flight, int keep_job, float *depth_out, float *normals_out,
    double *job_seconds, double *total_seconds, smvs_host_log *logs)
{
    return guarded([&] {
        require(mains != nullptr && subs_in != nullptr && o != nullptr && n_jobs >= 1
            && n_subs >= 1 && num_devices >= 1 && views_in_flight >= 1,
            "smvs_host_optimize_views: bad argument");
        Bundle::Ptr bundle = make_bundle(bundle_in);
        typedef std::chrono::steady_clock Clock;
        // per-phase wall time over all tasks (stderr with SMVS_HOST_TIMING)
        static const char *const phase_names[5] = { "StereoView::create x (1 + subs)",
            "SGM front end", "DepthOptimizer ctor", "optimize()", "maps for the caller (one job)" };
        std::mutex phase_lock;
        double phase_s[5] = { 0, 0, 0, 0, 0 };
        auto lap = [&](Clock::time_point& from, int phase) {
            Clock::time_point const now = Clock::now();
            std::lock_guard<std::mutex> guard(phase_lock);
            phase_s[phase] += std::chrono::duration<double>(now - from).count();
            from = now;
        };
        std::vector<std::future<void>> done;
        Clock::time_point const t_start = Clock::now();
        {
            ViewQueue queue(num_devices, views_in_flight);
            for (int job = 0; job < n_jobs; ++job)
                done.push_back(queue.add_task([=, &lap](ViewQueue::Slot const& slot) {
                    // app/smvsrecon.cc:662-732
                    Clock::time_point const t0 = Clock::now();
                    Clock::time_point tp = t0;
                    StereoView::Ptr main_view = make_view(mains[job], o->use_shading != 0);
                    std::vector<StereoView::Ptr> subs = make_views(
                        subs_in + (std::size_t)job * n_subs, n_subs);
                    lap(tp, 0);
                    DepthOptimizer::Options opts = optimizer_options(*o);
                    opts.device = first_device + slot.device;
                    opts.use_sgm = sgm_scale >= 0;
                    if (opts.use_sgm) {
                        SGMStereo::Options sgm_opts;
                        sgm_opts.scale = sgm_scale;
                        sgm_opts.device = opts.device;
                        (void)reconstruct_sgm_depth_for_view(sgm_opts, main_view, subs,
                            bundle);
                    }
                    lap(tp, 1);
                    DepthOptimizer optimizer(main_view, subs, bundle, opts);
                    lap(tp, 2);
                    optimizer.optimize();
                    lap(tp, 3);
                    // (optimize() has written the depth / normal embeddings,
                    // lib/depth_optimizer.cc:158-161; the maps are fetched once
                    // more only for the job whose result the caller wants)
                    if (job == keep_job)
                        copy_maps(optimizer, (std::size_t)mains[job].width * mains[job].height,
                            depth_out, normals_out);
                    lap(tp, 4);
                    if (logs != nullptr)
                        fill_log(optimizer, &logs[job]);
                    if (job_seconds != nullptr)
                        job_seconds[job] = std::chrono::duration<double>(
                            Clock::now() - t0).count();
                }));
            queue.wait_idle();
        }
        if (total_seconds != nullptr)
            *total_seconds = std::chrono::duration<double>(Clock::now() - t_start).count();
        if (std::getenv("SMVS_HOST_TIMING") != nullptr)
            for (int i = 0; i < 5; ++i)
                std::fprintf(stderr, "[smvs views] %-34s %8.2f ms per view\n",
                    phase_names[i], 1e3 * phase_s[i] / n_jobs);
        for (auto& f : done)
            f.get();   // rethrows a task's exception
    });
}

extern "C" int
smvs_host_view_queue_selftest(int n_tasks, int num_devices, int views_in_flight,
    int throwing_task, int *device_hist, int *worker_hist)
{
    return guarded([&] {
        require(n_tasks >= 0 && device_hist != nullptr && worker_hist != nullptr,
            "smvs_host_view_queue_selftest: bad argument");
        std::vector<int> ran(n_tasks, 0), on_device(n_tasks, -1), on_worker(n_tasks, -1);
        std::vector<std::future<void>> done;
        {
            ViewQueue queue(num_devices, views_in_flight);
            if (queue.num_workers() != num_devices * views_in_flight)
                throw std::logic_error("ViewQueue: wrong number of workers");
            for (int i = 0; i < n_tasks; ++i)
                done.push_back(queue.add_task([&, i](ViewQueue::Slot const& slot) {
                    ran[i] += 1;
                    on_device[i] = slot.device;
                    on_worker[i] = slot.worker;
                    std::this_thread::sleep_for(std::chrono::milliseconds(2));
                    if (i == throwing_task)
                        throw std::runtime_error("task failed on purpose");
                }));
            queue.wait_idle();
        }
        std::fill(device_hist, device_hist + num_devices, 0);
        std::fill(worker_hist, worker_hist + num_devices * views_in_flight, 0);
        for (int i = 0; i < n_tasks; ++i) {
            bool threw = false;
            try {
                done[i].get();
            } catch (std::runtime_error const&) {
                threw = true;
            }
            if (threw != (i == throwing_task))
                throw std::logic_error("ViewQueue: exception on the wrong future");
            if (ran[i] != 1 || on_device[i] < 0 || on_device[i] >= num_devices)
                throw std::logic_error("ViewQueue: a task did not run exactly once");
            if (on_worker[i] % num_devices != on_device[i])
                throw std::logic_error("ViewQueue: worker / device binding");
            device_hist[on_device[i]] += 1;
            worker_hist[on_worker[i]] += 1;
        }
    });
}

extern "C" int
smvs_host_gn_solve_step(const smvs_host_view *main_in, const smvs_host_view *subs_in,
    int n_subs, const smvs_host_bundle *bundle_in, int init_scale,
    double regularization, int device, float *main_grad, float *sub_grad,
    float *sub_hess, double *Mi_out, double *ti_out, float *flen2, double *g_out,
    double *x_out, double *H9_out, double *P_out, int *cg_out)
{
    return guarded([&] {
        require(main_in != nullptr && subs_in != nullptr && n_subs >= 1,
            "smvs_host_gn_solve_step: bad argument");
        StereoView::Ptr main_view = make_view(*main_in);
        std::vector<StereoView::Ptr> subs = make_views(subs_in, n_subs);
        Bundle::Ptr bundle = make_bundle(bundle_in);
        Surface::Ptr surface = Surface::create(bundle, main_view, init_scale);
        // lib/depth_optimizer.cc:63-66
        main_view->set_scale(surface->get_scale());
        for (auto& v : subs)
            v->set_scale(surface->get_scale());
        // lib/depth_optimizer.cc:679-699
        std::vector<Matrix3d> Mi(n_subs);
        std::vector<Vec3d> ti(n_subs);
        for (int j = 0; j < n_subs; ++j) {
            float M[9], t[3];
            main_view->get_camera().fill_reprojection(subs[j]->get_camera(),
                (float)main_view->get_width(), (float)main_view->get_height(),
                (float)subs[j]->get_width(), (float)subs[j]->get_height(), M, t);
            for (int k = 0; k < 9; ++k)
                Mi[j].m[k] = M[k];
            for (int k = 0; k < 3; ++k)
                ti[j].v[k] = t[k];
        }
        std::size_t const N = surface->get_num_nodes(), Pn = surface->get_num_patches();
        std::vector<std::vector<std::size_t>> subsurfaces(Pn);
        for (std::size_t p = 0; p < Pn; ++p)
            if (surface->patch_validity()[p])
                for (int j = 0; j < n_subs; ++j)
                    subsurfaces[p].push_back((std::size_t)j);
        std::vector<char> active(N);
        for (std::size_t n = 0; n < N; ++n)
            active[n] = surface->node_validity()[n] ? 1 : 0;

        GaussNewtonStep::Options gn_opts;
        gn_opts.regularization = regularization;
        gn_opts.device = device;
        GaussNewtonStep gauss_newton_step(gn_opts, main_view, subs, Mi, ti);
        GaussNewtonStep::SparseMatrix hessian, precond;
        GaussNewtonStep::DenseVector gradient;
        gauss_newton_step.construct(surface, subsurfaces, active, nullptr,
            &hessian, &gradient, &precond);
        // lib/depth_optimizer.cc:245-254
        double norm = 0.0;
        for (double v : gradient)
            norm += v * v;
        ConjugateGradient::Options cg_opts;
        cg_opts.error_tolerance = std::sqrt(norm) * 0.01;
        cg_opts.max_iterations = 200;
        ConjugateGradient cg(cg_opts, device);
        ConjugateGradient::Vector b(gradient.size()), delta;
        for (std::size_t i = 0; i < b.size(); ++i)
            b[i] = -gradient[i];
        ConjugateGradient::Status const status = cg.solve(hessian, b, &delta, &precond);

        std::size_t const npix = (std::size_t)main_in->width * main_in->height;
        if (main_grad != nullptr)
            std::memcpy(main_grad, main_view->get_image_gradients()->begin(),
                sizeof(float) * 2 * npix);
        for (int j = 0; j < n_subs; ++j) {
            std::size_t const sp = (std::size_t)subs[j]->get_width() * subs[j]->get_height();
            require(sp == npix, "smvs_host_gn_solve_step: the planes "
                "are returned for neighbours of the main view's size");
            if (sub_grad != nullptr)
                std::memcpy(sub_grad + 2 * npix * j,
                    subs[j]->get_image_gradients()->begin(), sizeof(float) * 2 * npix);
            if (sub_hess != nullptr)
                std::memcpy(sub_hess + 3 * npix * j,
                    subs[j]->get_image_hessian()->begin(), sizeof(float) * 3 * npix);
            if (Mi_out != nullptr)
                std::copy(Mi[j].m, Mi[j].m + 9, Mi_out + 9 * j);
            if (ti_out != nullptr)
                std::copy(ti[j].v, ti[j].v + 3, ti_out + 3 * j);
        }
        if (flen2 != nullptr) {
            flen2[0] = main_view->get_flen();
            flen2[1] = main_view->get_inverse_flen();
        }
        if (g_out != nullptr)
            std::copy(gradient.begin(), gradient.end(), g_out);
        if (x_out != nullptr)
            std::copy(delta.begin(), delta.end(), x_out);
        if (H9_out != nullptr)
            std::copy(hessian.blocks.begin(), hessian.blocks.end(), H9_out);
        if (P_out != nullptr)
            for (std::size_t n = 0; n < N; ++n)
                std::copy(precond.blocks.begin() + (n * 9 + 4) * 16,
                    precond.blocks.begin() + (n * 9 + 5) * 16, P_out + n * 16);
        if (cg_out != nullptr) {
            cg_out[0] = status.num_iterations;
            cg_out[1] = (int)status.info;
        }
    });
}

extern "C" int
smvs_host_block_multiply(int num_nodes, int node_stride, const double *blocks9,
    const double *x, double *y)
{
    return guarded([&] {
        require(num_nodes >= 1 && node_stride >= 1 && blocks9 != nullptr && x != nullptr
            && y != nullptr, "smvs_host_block_multiply: bad argument");
        BlockStencilMatrix A;
        A.num_nodes = (std::size_t)num_nodes;
        A.node_stride = (std::size_t)node_stride;
        A.blocks.assign(blocks9, blocks9 + (std::size_t)num_nodes * 9 * 16);
        ConjugateGradient::Functor const& op = A;      // (through the interface)
        ConjugateGradient::Vector const r = op.multiply(
            ConjugateGradient::Vector(x, x + 4 * (std::size_t)num_nodes));
        std::copy(r.begin(), r.end(), y);
    });
}
