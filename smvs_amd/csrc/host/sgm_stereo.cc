#include "sgm_stereo.h"

#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <string>

#include "../../../include/smvs_hip.h"

namespace smvs_amd {

namespace {

// the two switches the reference's Options do not have, as the device takes them
smvs_sgm_options
device_options(SGMStereo::Options const& o)
{
    smvs_sgm_options d;
    d.p2_mode = o.adaptive_penalty2 ? SMVS_SGM_P2_ADAPTIVE : SMVS_SGM_P2_CONSTANT;
    d.winner = o.subplane ? SMVS_SGM_WINNER_SUBPLANE : SMVS_SGM_WINNER_PLANE;
    return d;
}

// a device entry's answer: its error under the name of the entry called
void
require_ok(int rc, char const* entry)
{
    if (rc != SMVS_OK)
        throw std::runtime_error(std::string(entry) + ": " + smvs_last_error());
}
#define SGM_DEVICE_CALL(entry, ...) require_ok(entry(__VA_ARGS__), #entry)

} // namespace

SGMStereo::SGMStereo(Options const& opts, StereoView::Ptr main,
    StereoView::Ptr neighbor)
    : opts(opts), main(main), neighbor(neighbor)
{
    // lib/sgm_stereo.cc:27-44
    this->main_image = main->get_byte_image();
    for (int i = 0; i < opts.scale; ++i)
        this->main_image = imgtools::rescale_half_size(this->main_image);
    this->neighbor_image = neighbor->get_byte_image();
    for (int i = 0; i < opts.scale; ++i)
        this->neighbor_image = imgtools::rescale_half_size(this->neighbor_image);
}

FloatImage::Ptr
SGMStereo::run_sgm(float min_depth, float max_depth)
{
    // lib/sgm_stereo.cc:98-124 on the device
    float M[9], t[3];
    this->main->get_camera().fill_reprojection(this->neighbor->get_camera(),
        (float)main_image->width(), (float)main_image->height(),
        (float)neighbor_image->width(), (float)neighbor_image->height(), M, t);
    FloatImage::Ptr depth = FloatImage::create(main_image->width(),
        main_image->height(), 1);
    smvs_sgm_options const dev_opts = device_options(opts);
    SGM_DEVICE_CALL(smvs_sgm_run_opts, opts.device, main_image->begin(),
        main_image->width(), main_image->height(), neighbor_image->begin(),
        neighbor_image->width(), neighbor_image->height(), M, t, min_depth,
        max_depth, opts.num_steps, opts.penalty1, opts.penalty2, &dev_opts,
        depth->begin(), nullptr, nullptr, nullptr);
    return depth;
}

void
SGMStereo::fill_depth_range_for_view(Bundle::ConstPtr bundle,
    StereoView::Ptr view, float* range)
{
    // lib/sgm_stereo.cc:669-720
    std::vector<float> depth_values;
    int const width = view->get_width(), height = view->get_height();
    CameraInfo const& cam = view->get_camera();
    double const fwidth2 = (double)width / 2.0, fheight2 = (double)height / 2.0;
    double const fnorm = (double)std::max(width, height);
    for (auto const& feat : bundle->features)
        for (int vid : feat.view_ids)
            if (vid == view->get_view_id()) {
                float proj[3];
                for (int r = 0; r < 3; ++r)
                    proj[r] = cam.rot[3 * r] * feat.pos[0]
                        + cam.rot[3 * r + 1] * feat.pos[1]
                        + cam.rot[3 * r + 2] * feat.pos[2] + cam.trans[r];
                float const depth = proj[2];
                proj[0] = proj[0] * cam.flen / proj[2];
                proj[1] = proj[1] * cam.flen / proj[2];
                float const ix = (float)(proj[0] * fnorm + fwidth2);
                float const iy = (float)(proj[1] * fnorm + fheight2);
                int const x = (int)std::floor(ix), y = (int)std::floor(iy);
                if (x >= 0 && x < width && y >= 0 && y < height)
                    depth_values.push_back(depth);
                break;
            }
    std::sort(depth_values.begin(), depth_values.end());
    if (depth_values.size() < 2) {
        range[0] = 0.3f;
        range[1] = 1.1f;
    } else {
        range[0] = depth_values.front() * 0.7f;
        range[1] = (float)(depth_values[(depth_values.size() * 99) / 100] * 5.0);
    }
}

namespace {

// One (main, neighbour) pair as the device entry wants it: the neighbour's raw
// bytes (the device desaturates and halves them: SGMStereo's constructor,
// lib/sgm_stereo.cc:27-39), both reprojections at the SGM-scale sizes and both
// depth ranges (lib/sgm_stereo.cc:46-62).
struct PairInputs {
    ByteImage::ConstPtr neighbor_bytes;
    int channels;
    smvs_sgm_neighbor dev;
};

void
sgm_scale_size(int scale, int* w, int* h)
{
    for (int i = 0; i < scale; ++i) {
        *w = (*w + 1) >> 1;
        *h = (*h + 1) >> 1;
    }
}

void
prepare_pair(SGMStereo::Options const& o, StereoView::Ptr main_view,
    StereoView::Ptr neighbor, Bundle::ConstPtr bundle, PairInputs* out)
{
    out->neighbor_bytes = neighbor->get_raw_bytes();
    out->channels = out->neighbor_bytes->channels();
    smvs_sgm_neighbor& d = out->dev;
    d.image = out->neighbor_bytes->begin();
    d.width = out->neighbor_bytes->width();      // full resolution
    d.height = out->neighbor_bytes->height();
    int mwi = main_view->get_width(), mhi = main_view->get_height();
    int nwi = d.width, nhi = d.height;
    sgm_scale_size(o.scale, &mwi, &mhi);
    sgm_scale_size(o.scale, &nwi, &nhi);
    float const mw = (float)mwi, mh = (float)mhi, nw = (float)nwi, nh = (float)nhi;
    main_view->get_camera().fill_reprojection(neighbor->get_camera(), mw, mh,
        nw, nh, d.M_fwd, d.t_fwd);
    neighbor->get_camera().fill_reprojection(main_view->get_camera(), nw, nh,
        mw, mh, d.M_bwd, d.t_bwd);
    d.range_main[0] = d.range_neighbor[0] = o.min_depth;
    d.range_main[1] = d.range_neighbor[1] = o.max_depth;
    if (bundle != nullptr && o.max_depth == 0.0) {
        SGMStereo::fill_depth_range_for_view(bundle, main_view, d.range_main);
        SGMStereo::fill_depth_range_for_view(bundle, neighbor, d.range_neighbor);
    }
}

// pairs: the n_front neighbours of the front end, then the further witnesses
// of the photo-consistency test (none with the test off); *confidence: its map
// when it is on; *slant: the two slants of the refinement sweeps when they are on
FloatImage::Ptr
run_pairs(SGMStereo::Options const& o, StereoView::Ptr main_view,
    std::vector<PairInputs> const& pairs, int n_front, FloatImage::Ptr* confidence,
    FloatImage::Ptr* slant)
{
    std::vector<smvs_sgm_neighbor> dev;
    std::vector<int> channels;
    for (auto const& p : pairs) {
        dev.push_back(p.dev);
        channels.push_back(p.channels);
    }
    ByteImage::ConstPtr main_bytes = main_view->get_raw_bytes();
    uint8_t const* const pixels = main_bytes->begin();
    int const fw = main_bytes->width(), fh = main_bytes->height();
    int const fc = main_bytes->channels(), n = n_front;
    int const n_witness = (int)dev.size() - n_front;
    int w = fw, h = fh;
    sgm_scale_size(o.scale, &w, &h);
    FloatImage::Ptr depth = FloatImage::create_for_overwrite(w, h, 1);
    // the option structs of every front; which entry is called: the sweep, the
    // consensus, the filters (their defaults call the entries without them)
    smvs_sgm_options const base = device_options(o);
    smvs_sgm_view_options const view_opts = { base.p2_mode, base.winner,
        o.consensus ? SMVS_SGM_MERGE_CONSENSUS : SMVS_SGM_MERGE_REFERENCE, o.min_agree,
        o.agree_ratio };
    smvs_sgm_sweep_options const sweep_opts = { base.p2_mode, base.winner,
        o.sweep_min_views < 0 ? std::min(2, n) : o.sweep_min_views,
        o.sweep_best_k < 0 ? (n + 1) / 2 : o.sweep_best_k, o.sweep_support_cost,
        o.sweep_min_support < 0 ? std::min(2, n) : o.sweep_min_support };
    smvs_sgm_filter_options const filter = { o.uniqueness, o.uniqueness_window,
        o.speckle_size, o.speckle_ratio };
    bool const filtered = !o.filters_default();
    smvs_sgm_photo_options const photo = { o.photo_radius, o.photo_best_k, o.photo_min_views,
        o.photo_min_score };
    smvs_sgm_refine_options const refine = { o.refine_sweeps, o.refine_samples,
        o.refine_depth_step, o.refine_slant_step, o.refine_seed, o.refine_fill };
    if (!o.refine_default()) {
        // the sweeps in the test's place (sweeps 0: the test, or nothing); the
        // device refuses sweeps without the test
        if (o.photo_radius != 0)
            *confidence = FloatImage::create_for_overwrite(w, h, 1);
        if (o.refine_sweeps != 0)
            *slant = FloatImage::create_for_overwrite(w, h, 2);
        float* const conf = *confidence != nullptr ? (*confidence)->begin() : nullptr;
        float* const sl = *slant != nullptr ? (*slant)->begin() : nullptr;
        if (o.sweep)
            SGM_DEVICE_CALL(smvs_sgm_sweep_for_view_raw_refine, o.device, pixels, fw, fh, fc,
                dev.data(), channels.data(), n, o.scale, dev[0].range_main, o.num_steps,
                o.penalty1, o.penalty2, &sweep_opts, &filter, depth->begin(), nullptr, nullptr,
                nullptr, nullptr, nullptr, n_witness, &photo, conf, nullptr, &refine, sl);
        else
            SGM_DEVICE_CALL(smvs_sgm_depth_for_view_raw_refine, o.device, pixels, fw, fh, fc,
                dev.data(), channels.data(), n, o.scale, o.num_steps, o.penalty1, o.penalty2,
                &view_opts, &filter, depth->begin(), nullptr, nullptr, n_witness, &photo,
                conf, nullptr, &refine, sl);
    } else if (o.photo_radius != 0) {
        // the test behind whichever front: the entries that take every option
        *confidence = FloatImage::create_for_overwrite(w, h, 1);
        if (o.sweep)
            SGM_DEVICE_CALL(smvs_sgm_sweep_for_view_raw_photo, o.device, pixels, fw, fh, fc,
                dev.data(), channels.data(), n, o.scale, dev[0].range_main, o.num_steps,
                o.penalty1, o.penalty2, &sweep_opts, &filter, depth->begin(), nullptr, nullptr,
                nullptr, nullptr, nullptr, n_witness, &photo, (*confidence)->begin(), nullptr);
        else
            SGM_DEVICE_CALL(smvs_sgm_depth_for_view_raw_photo, o.device, pixels, fw, fh, fc,
                dev.data(), channels.data(), n, o.scale, o.num_steps, o.penalty1, o.penalty2,
                &view_opts, &filter, depth->begin(), nullptr, nullptr, n_witness, &photo,
                (*confidence)->begin(), nullptr);
    } else if (o.sweep && filtered)
        // n x (warp + cost) over the main view's planes, one fold, one
        // aggregation, one winner, the support test
        SGM_DEVICE_CALL(smvs_sgm_sweep_for_view_raw_filtered, o.device, pixels, fw, fh, fc,
            dev.data(), channels.data(), n, o.scale, dev[0].range_main, o.num_steps, o.penalty1,
            o.penalty2, &sweep_opts, &filter, depth->begin(), nullptr);
    else if (o.sweep)
        SGM_DEVICE_CALL(smvs_sgm_sweep_for_view_raw, o.device, pixels, fw, fh, fc, dev.data(),
            channels.data(), n, o.scale, dev[0].range_main, o.num_steps, o.penalty1, o.penalty2,
            &sweep_opts, depth->begin(), nullptr);
    else if (filtered)
        // with the filters either merge goes through the one entry that takes them
        SGM_DEVICE_CALL(smvs_sgm_depth_for_view_raw_filtered, o.device, pixels, fw, fh, fc,
            dev.data(), channels.data(), n, o.scale, o.num_steps, o.penalty1, o.penalty2,
            &view_opts, &filter, depth->begin(), nullptr, nullptr);
    else if (o.consensus)
        // 2 n x run_sgm, then the n checks and the consensus in one kernel
        SGM_DEVICE_CALL(smvs_sgm_depth_for_view_raw_merge, o.device, pixels, fw, fh, fc,
            dev.data(), channels.data(), n, o.scale, o.num_steps, o.penalty1, o.penalty2,
            &view_opts, depth->begin(), nullptr, nullptr);
    else
        // desaturate + half-size on the device, then 4 x run_sgm, L/R check, merge
        SGM_DEVICE_CALL(smvs_sgm_depth_for_view_raw_opts, o.device, pixels, fw, fh, fc,
            dev.data(), channels.data(), n, o.scale, o.num_steps, o.penalty1, o.penalty2, &base,
            depth->begin());
    return depth;
}

} // namespace

FloatImage::Ptr
SGMStereo::reconstruct(Options sgm_opts, StereoView::Ptr main_view,
    StereoView::Ptr neighbor, Bundle::ConstPtr bundle)
{
    // lib/sgm_stereo.cc:46-96: both run_sgm calls and the left / right
    // consistency check on the device
    std::vector<PairInputs> pairs(1);
    prepare_pair(sgm_opts, main_view, neighbor, bundle, &pairs[0]);
    sgm_opts.photo_radius = 0;      // (a pair has no further witness)
    sgm_opts.refine_sweeps = 0;
    FloatImage::Ptr confidence, slant;
    return run_pairs(sgm_opts, main_view, pairs, 1, &confidence, &slant);
}

FloatImage::Ptr
reconstruct_sgm_depth_for_view(SGMStereo::Options opts,
    StereoView::Ptr main_view, std::vector<StereoView::Ptr> const& neighbors,
    Bundle::ConstPtr bundle)
{
    // app/smvsrecon.cc:346-384: SGMStereo::reconstruct against the first two
    // neighbours and the merge of the two checked maps, in one device call;
    // with opts.consensus or opts.sweep against the first opts.num_neighbors
    if (neighbors.empty())
        throw std::invalid_argument("reconstruct_sgm_depth_for_view: no neighbour");
    if (opts.num_neighbors < 1 || opts.num_neighbors > SMVS_MAX_SUBS)
        throw std::invalid_argument("reconstruct_sgm_depth_for_view: num_neighbors "
            "must be in [1, " + std::to_string(SMVS_MAX_SUBS) + "]");
    if (opts.sweep && opts.consensus)
        throw std::invalid_argument("reconstruct_sgm_depth_for_view: Options::sweep and "
            "Options::consensus exclude each other");
    if (!opts.consensus && !opts.sweep && opts.num_neighbors > 2)
        throw std::invalid_argument("reconstruct_sgm_depth_for_view: the reference's "
            "merge takes one or two neighbours (app/smvsrecon.cc:360-365); more need "
            "Options::consensus or Options::sweep");
    std::size_t const n_front = std::min<std::size_t>(neighbors.size(),
        (std::size_t)opts.num_neighbors);
    // with the photo-consistency test: the first photo_witnesses neighbours (all
    // of them at -1, SMVS_MAX_SUBS at the most, the front's own at the least)
    std::size_t n_all = n_front;
    if (opts.photo_radius != 0) {
        std::size_t const asked = opts.photo_witnesses < 0 ? neighbors.size()
            : (std::size_t)opts.photo_witnesses;
        n_all = std::max(n_front, std::min<std::size_t>(std::min(asked, neighbors.size()),
            (std::size_t)SMVS_MAX_SUBS));
    }
    std::vector<PairInputs> pairs(n_all);
    for (std::size_t k = 0; k < pairs.size(); ++k)
        prepare_pair(opts, main_view, neighbors[k], bundle, &pairs[k]);
    FloatImage::Ptr confidence, slant;
    FloatImage::Ptr d1 = run_pairs(opts, main_view, pairs, (int)n_front, &confidence, &slant);
    if (confidence != nullptr)
        main_view->write_image_to_view(confidence, "smvs-sgm-confidence");
    if (slant != nullptr)
        main_view->write_image_to_view(slant, "smvs-sgm-slant");
    // (app/smvsrecon.cc:383: write_depth_to_view -- the conversion of the stored
    // copy to MVE's convention waits until the embedding is read; the optimizer
    // of this view takes the map as it is and converts on the device)
    main_view->write_depth_to_view_deferred(d1, "smvs-sgm");
    return d1;
}

} // namespace smvs_amd
