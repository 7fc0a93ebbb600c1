// C ABI of the host mirror (host_capi.h): the SGM front end of one view -- the
// one conversion of the C side into SGMStereo::Options, the checks the scene
// entries share with it, the defaults, smvs_host_sgm_depth_* -- and the
// front end's host-only pieces.
#include "capi_internal.h"

#include "scene_io.h"

using namespace smvs_amd;
using namespace smvs_amd::capi;

SGMStereo::Options
smvs_amd::capi::sgm_options(SgmArgs const& a, bool adaptive_penalty2)
{
    SGMStereo::Options opts;
    opts.num_steps = a.num_steps;
    opts.adaptive_penalty2 = adaptive_penalty2;
    opts.subplane = a.subplane != 0;
    opts.num_neighbors = a.num_neighbors;
    opts.consensus = a.consensus != 0;
    opts.agree_ratio = a.agree_ratio;
    opts.min_agree = a.min_agree;
    if (a.sweep_on()) {
        opts.sweep = true;
        opts.sweep_min_views = a.sweep->min_views;
        opts.sweep_best_k = a.sweep->best_k;
        opts.sweep_support_cost = a.sweep->support_cost;
        opts.sweep_min_support = a.sweep->min_support;
    }
    if (a.filter != nullptr) {
        opts.uniqueness = a.filter->uniqueness;
        opts.uniqueness_window = a.filter->uniqueness_window;
        opts.speckle_size = a.filter->speckle_size;
        opts.speckle_ratio = a.filter->speckle_ratio;
    }
    if (a.photo != nullptr) {
        opts.photo_radius = a.photo->radius;
        opts.photo_best_k = a.photo->best_k;
        opts.photo_min_views = a.photo->min_views;
        opts.photo_min_score = a.photo->min_score;
        opts.photo_witnesses = a.photo->witnesses;
    }
    if (a.refine != nullptr) {
        opts.refine_sweeps = a.refine->sweeps;
        opts.refine_samples = a.refine->samples;
        opts.refine_depth_step = a.refine->depth_step;
        opts.refine_slant_step = a.refine->slant_step;
        opts.refine_seed = a.refine->seed;
        opts.refine_fill = a.refine->fill;
    }
    return opts;
}

// The accepted sets of include/smvs_hip.h, the photo test's as far as it does
// not depend on the witnesses there are (a NaN fails the comparisons); sweeps
// without the photo test: the device refuses them.
void
smvs_amd::capi::check_sgm_records(SgmArgs const& a, std::string const& family)
{
    if (const smvs_host_sgm_filter *f = a.filter)
        require(f->uniqueness >= 0 && f->uniqueness <= 99 && f->uniqueness_window >= 1
            && f->uniqueness_window <= 256 && f->speckle_size >= 0
            && f->speckle_ratio >= 0.0f && f->speckle_ratio <= 1.0f,
            family + "_filtered: sgm_uniqueness must be in [0, 99], "
            "sgm_uniqueness_window in [1, 256], sgm_speckle_size not negative and "
            "sgm_speckle_ratio in [0, 1]");
    if (const smvs_host_sgm_photo *p = a.photo)
        require(p->radius >= 0 && p->radius <= 3 && p->best_k >= 0 && p->best_k <= SMVS_MAX_SUBS
            && p->min_views >= 0 && p->min_views <= SMVS_MAX_SUBS
            && p->min_score >= -1.0f && p->min_score <= 1.0f && p->witnesses >= -1
            && p->witnesses <= SMVS_MAX_SUBS,
            family + "_photo: sgm_photo_radius must be in [0, 3], "
            "sgm_photo_best_k and sgm_photo_min_views in [0, 16], sgm_photo_min_score in "
            "[-1, 1] and sgm_photo_witnesses -1 or in [0, 16]");
    if (const smvs_host_sgm_refine *r = a.refine)
        require(r->sweeps >= 0 && r->sweeps <= 8 && r->samples >= 0 && r->samples <= 8
            && r->depth_step >= 0.0f && r->depth_step <= 1.0f
            && r->slant_step >= 0.0f && r->slant_step <= 1.0f && (r->fill == 0 || r->fill == 1),
            family + "_refine: sgm_refine_sweeps and "
            "sgm_refine_samples must be in [0, 8], sgm_refine_depth_step and "
            "sgm_refine_slant_step in [0, 1] and sgm_refine_fill 0 or 1");
}

// ---------------------------------------------------------------- defaults
// Each getter reports a default-constructed SGMStereo::Options in the first half
// of its arrays and the one a default-constructed ReconSettings holds in the
// second, slot for slot.
namespace {

struct BothDefaults
{
    SGMStereo::Options of[2] = { SGMStereo::Options(), ReconSettings().sgm };
};

// k-th half of an array of 2 * n ints
template <int n> void
put(int *out, int k, int const (&values)[n])
{
    std::copy(values, values + n, out + n * k);
}

} // namespace

extern "C" int
smvs_host_sgm_default_switches(int *out4)
{
    return guarded([&] {
        require(out4 != nullptr, "smvs_host_sgm_default_switches: bad argument");
        BothDefaults const both{};
        for (int k = 0; k < 2; ++k)
            put(out4, k, { both.of[k].adaptive_penalty2, both.of[k].subplane });
    });
}

extern "C" int
smvs_host_sgm_merge_defaults(int *ints8, float *ratios2)
{
    return guarded([&] {
        require(ints8 != nullptr && ratios2 != nullptr,
            "smvs_host_sgm_merge_defaults: bad argument");
        BothDefaults const both{};
        for (int k = 0; k < 2; ++k) {
            SGMStereo::Options const& o = both.of[k];
            put(ints8, k, { o.num_neighbors, o.consensus, o.min_agree, 0 });
            ratios2[k] = o.agree_ratio;
        }
    });
}

extern "C" int
smvs_host_sgm_sweep_defaults(int *ints10)
{
    return guarded([&] {
        require(ints10 != nullptr, "smvs_host_sgm_sweep_defaults: bad argument");
        BothDefaults const both{};
        for (int k = 0; k < 2; ++k) {
            SGMStereo::Options const& o = both.of[k];
            put(ints10, k, { o.sweep, o.sweep_min_views, o.sweep_best_k, o.sweep_support_cost,
                o.sweep_min_support });
        }
    });
}

extern "C" int
smvs_host_sgm_filter_defaults(int *ints6, float *ratios2)
{
    return guarded([&] {
        require(ints6 != nullptr && ratios2 != nullptr,
            "smvs_host_sgm_filter_defaults: bad argument");
        BothDefaults const both{};
        for (int k = 0; k < 2; ++k) {
            SGMStereo::Options const& o = both.of[k];
            put(ints6, k, { o.uniqueness, o.uniqueness_window, o.speckle_size });
            ratios2[k] = o.speckle_ratio;
        }
    });
}

extern "C" int
smvs_host_sgm_refine_defaults(int *ints8, float *steps4)
{
    return guarded([&] {
        require(ints8 != nullptr && steps4 != nullptr,
            "smvs_host_sgm_refine_defaults: bad argument");
        BothDefaults const both{};
        for (int k = 0; k < 2; ++k) {
            SGMStereo::Options const& o = both.of[k];
            put(ints8, k, { o.refine_sweeps, o.refine_samples, (int)o.refine_seed,
                o.refine_fill });
            steps4[2 * k] = o.refine_depth_step;
            steps4[2 * k + 1] = o.refine_slant_step;
        }
    });
}

extern "C" int
smvs_host_sgm_photo_defaults(int *ints8, float *scores2)
{
    return guarded([&] {
        require(ints8 != nullptr && scores2 != nullptr,
            "smvs_host_sgm_photo_defaults: bad argument");
        BothDefaults const both{};
        for (int k = 0; k < 2; ++k) {
            SGMStereo::Options const& o = both.of[k];
            put(ints8, k, { o.photo_radius, o.photo_best_k, o.photo_min_views,
                o.photo_witnesses });
            scores2[k] = o.photo_min_score;
        }
    });
}

// ------------------------------------------------------ smvs_host_sgm_depth_*
namespace {

// One call of the family: what smvs_host_sgm_depth takes, then what the later
// entries added, each with the value the entries before it run with.
struct SgmDepthCall
{
    const smvs_host_view *main_in, *subs_in;
    int n_subs;
    const smvs_host_bundle *bundle_in;
    int sgm_scale;
    float min_depth, max_depth;
    int device;
    float *depth_out;
    int *out_w, *out_h;
    int adaptive_penalty2 = SGMStereo::Options().adaptive_penalty2;
    SgmArgs sgm;
    float *confidence_out = nullptr, *slant_out = nullptr;
};

int
sgm_depth(SgmDepthCall const& c)
{
    return guarded([&] {
        // (before the views are copied: an argument error needs no image)
        check_sgm_records(c.sgm, "smvs_host_sgm_depth");
        require(!(c.sgm.sweep_on() && c.sgm.consensus != 0),
            "smvs_host_sgm_depth_sweep: sweep and consensus exclude each other");
        require(c.sgm.consensus != 0 || c.sgm.sweep_on() || c.sgm.num_neighbors <= 2,
            "smvs_host_sgm_depth_merge: more than two neighbours need the consensus merge "
            "or the sweep");
        require(SGMStereo::Options::valid_num_steps(c.sgm.num_steps),
            "smvs_host_sgm_depth_steps: num_steps must be in [2, 128] or a multiple of 8 "
            "in [136, 256]");
        StereoView::Ptr main_view = make_view(*c.main_in);
        std::vector<StereoView::Ptr> subs = make_views(c.subs_in, c.n_subs);
        SGMStereo::Options opts = sgm_options(c.sgm, c.adaptive_penalty2 != 0);
        opts.scale = c.sgm_scale;
        opts.min_depth = c.min_depth;
        opts.max_depth = c.max_depth;
        opts.device = c.device;
        FloatImage::Ptr d = reconstruct_sgm_depth_for_view(opts, main_view, subs,
            make_bundle(c.bundle_in));
        if (c.slant_out != nullptr && main_view->has_embedding("smvs-sgm-slant")) {
            FloatImage::Ptr s = main_view->get_embedding("smvs-sgm-slant");
            std::memcpy(c.slant_out, s->begin(),
                sizeof(float) * s->get_pixel_amount() * s->channels());
        }
        if (c.confidence_out != nullptr && main_view->has_embedding("smvs-sgm-confidence")) {
            FloatImage::Ptr s = main_view->get_embedding("smvs-sgm-confidence");
            std::memcpy(c.confidence_out, s->begin(), sizeof(float) * s->get_pixel_amount());
        }
        if (c.out_w != nullptr)
            *c.out_w = d->width();
        if (c.out_h != nullptr)
            *c.out_h = d->height();
        if (c.depth_out != nullptr)
            std::memcpy(c.depth_out, d->begin(), sizeof(float) * d->get_pixel_amount());
    });
}

} // namespace

extern "C" int
smvs_host_sgm_depth(const smvs_host_view *main_in, const smvs_host_view *subs_in,
    int n_subs, const smvs_host_bundle *bundle_in, int sgm_scale,
    float min_depth, float max_depth, int device, float *depth_out, int *out_w,
    int *out_h)
{
    return sgm_depth({ main_in, subs_in, n_subs, bundle_in, sgm_scale, min_depth, max_depth,
        device, depth_out, out_w, out_h });
}

extern "C" int
smvs_host_sgm_depth_mode(const smvs_host_view *main_in, const smvs_host_view *subs_in,
    int n_subs, const smvs_host_bundle *bundle_in, int sgm_scale,
    float min_depth, float max_depth, int device, int adaptive_penalty2,
    float *depth_out, int *out_w, int *out_h)
{
    return sgm_depth({ main_in, subs_in, n_subs, bundle_in, sgm_scale, min_depth, max_depth,
        device, depth_out, out_w, out_h, adaptive_penalty2 });
}

extern "C" int
smvs_host_sgm_depth_steps(const smvs_host_view *main_in, const smvs_host_view *subs_in,
    int n_subs, const smvs_host_bundle *bundle_in, int sgm_scale,
    float min_depth, float max_depth, int device, int adaptive_penalty2,
    int num_steps, float *depth_out, int *out_w, int *out_h)
{
    return sgm_depth({ main_in, subs_in, n_subs, bundle_in, sgm_scale, min_depth, max_depth,
        device, depth_out, out_w, out_h, adaptive_penalty2, { num_steps } });
}

extern "C" int
smvs_host_sgm_depth_subplane(const smvs_host_view *main_in, const smvs_host_view *subs_in,
    int n_subs, const smvs_host_bundle *bundle_in, int sgm_scale,
    float min_depth, float max_depth, int device, int adaptive_penalty2,
    int num_steps, int subplane, float *depth_out, int *out_w, int *out_h)
{
    return sgm_depth({ main_in, subs_in, n_subs, bundle_in, sgm_scale, min_depth, max_depth,
        device, depth_out, out_w, out_h, adaptive_penalty2, { num_steps, subplane } });
}

extern "C" int
smvs_host_sgm_depth_merge(const smvs_host_view *main_in, const smvs_host_view *subs_in,
    int n_subs, const smvs_host_bundle *bundle_in, int sgm_scale,
    float min_depth, float max_depth, int device, int adaptive_penalty2,
    int num_steps, int subplane, int num_neighbors, int consensus, float agree_ratio,
    int min_agree, float *depth_out, int *out_w, int *out_h)
{
    return sgm_depth({ main_in, subs_in, n_subs, bundle_in, sgm_scale, min_depth, max_depth,
        device, depth_out, out_w, out_h, adaptive_penalty2, { num_steps, subplane,
            num_neighbors, consensus, agree_ratio, min_agree } });
}

extern "C" int
smvs_host_sgm_depth_sweep(const smvs_host_view *main_in, const smvs_host_view *subs_in,
    int n_subs, const smvs_host_bundle *bundle_in, int sgm_scale,
    float min_depth, float max_depth, int device, int adaptive_penalty2,
    int num_steps, int subplane, int num_neighbors, int consensus, float agree_ratio,
    int min_agree, const smvs_host_sgm_sweep *sweep, float *depth_out, int *out_w,
    int *out_h)
{
    return sgm_depth({ main_in, subs_in, n_subs, bundle_in, sgm_scale, min_depth, max_depth,
        device, depth_out, out_w, out_h, adaptive_penalty2, { num_steps, subplane,
            num_neighbors, consensus, agree_ratio, min_agree, sweep } });
}

extern "C" int
smvs_host_sgm_depth_filtered(const smvs_host_view *main_in, const smvs_host_view *subs_in,
    int n_subs, const smvs_host_bundle *bundle_in, int sgm_scale,
    float min_depth, float max_depth, int device, int adaptive_penalty2,
    int num_steps, int subplane, int num_neighbors, int consensus, float agree_ratio,
    int min_agree, const smvs_host_sgm_sweep *sweep, const smvs_host_sgm_filter *filter,
    float *depth_out, int *out_w, int *out_h)
{
    return sgm_depth({ main_in, subs_in, n_subs, bundle_in, sgm_scale, min_depth, max_depth,
        device, depth_out, out_w, out_h, adaptive_penalty2, { num_steps, subplane,
            num_neighbors, consensus, agree_ratio, min_agree, sweep, filter } });
}

extern "C" int
smvs_host_sgm_depth_photo(const smvs_host_view *main_in, const smvs_host_view *subs_in,
    int n_subs, const smvs_host_bundle *bundle_in, int sgm_scale,
    float min_depth, float max_depth, int device, int adaptive_penalty2,
    int num_steps, int subplane, int num_neighbors, int consensus, float agree_ratio,
    int min_agree, const smvs_host_sgm_sweep *sweep, const smvs_host_sgm_filter *filter,
    const smvs_host_sgm_photo *photo, float *depth_out, float *confidence_out, int *out_w,
    int *out_h)
{
    return sgm_depth({ main_in, subs_in, n_subs, bundle_in, sgm_scale, min_depth, max_depth,
        device, depth_out, out_w, out_h, adaptive_penalty2, { num_steps, subplane,
            num_neighbors, consensus, agree_ratio, min_agree, sweep, filter, photo },
        confidence_out });
}

extern "C" int
smvs_host_sgm_depth_refine(const smvs_host_view *main_in, const smvs_host_view *subs_in,
    int n_subs, const smvs_host_bundle *bundle_in, int sgm_scale,
    float min_depth, float max_depth, int device, int adaptive_penalty2,
    int num_steps, int subplane, int num_neighbors, int consensus, float agree_ratio,
    int min_agree, const smvs_host_sgm_sweep *sweep, const smvs_host_sgm_filter *filter,
    const smvs_host_sgm_photo *photo, const smvs_host_sgm_refine *refine, float *depth_out,
    float *confidence_out, float *slant_out, int *out_w, int *out_h)
{
    return sgm_depth({ main_in, subs_in, n_subs, bundle_in, sgm_scale, min_depth, max_depth,
        device, depth_out, out_w, out_h, adaptive_penalty2, { num_steps, subplane,
            num_neighbors, consensus, agree_ratio, min_agree, sweep, filter, photo, refine },
        confidence_out, slant_out });
}

// ------------------------------------------- host-only pieces of the front end
extern "C" int
smvs_host_depth_range(const smvs_host_view *view_in,
    const smvs_host_bundle *bundle_in, float *range2)
{
    return guarded([&] {
        require(view_in != nullptr && bundle_in != nullptr && range2 != nullptr,
            "smvs_host_depth_range: bad argument");
        StereoView::Ptr view = make_view(*view_in);
        SGMStereo::fill_depth_range_for_view(make_bundle(bundle_in), view, range2);
    });
}

extern "C" int
smvs_host_reprojection(const smvs_host_view *source,
    const smvs_host_view *destination, float *M9, float *t3)
{
    return guarded([&] {
        require(source != nullptr && destination != nullptr && M9 != nullptr && t3 != nullptr,
            "smvs_host_reprojection: bad argument");
        make_camera(*source).fill_reprojection(make_camera(*destination),
            (float)source->width, (float)source->height,
            (float)destination->width, (float)destination->height, M9, t3);
    });
}

extern "C" int
smvs_host_sgm_image(const smvs_host_view *view_in, int halvings, uint8_t *out,
    int *out_w, int *out_h)
{
    return guarded([&] {
        require(view_in != nullptr && out != nullptr && out_w != nullptr
            && out_h != nullptr && halvings >= 0, "smvs_host_sgm_image: bad argument");
        ByteImage::ConstPtr img = make_view(*view_in)->get_byte_image();
        for (int i = 0; i < halvings; ++i)
            img = imgtools::rescale_half_size(img);
        *out_w = img->width();
        *out_h = img->height();
        std::memcpy(out, img->begin(), (std::size_t)img->width() * img->height());
    });
}
