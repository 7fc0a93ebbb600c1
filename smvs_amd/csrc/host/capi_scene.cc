// C ABI of the host mirror (host_capi.h): smvsrecon's scene-level run and what
// goes with a scene on disk -- its description, neighbour selection, and the
// byte-image containers of a view directory.
#include "capi_internal.h"

#include "jpeg_io.h"
#include "png_io.h"
#include "scene_io.h"
#include "view_selection.h"

using namespace smvs_amd;
using namespace smvs_amd::capi;

namespace {

// the flag bits of the entries up to smvs_host_reconstruct_scene_refine
unsigned const SCENE_FLAGS_REFINE = SMVS_HOST_SCENE_ADAPTIVE_PENALTY2
    | SMVS_HOST_SCENE_DEVICE_INPUT_SCALING | SMVS_HOST_SCENE_DEVICE_SHADING_PREP
    | SMVS_HOST_SCENE_GAMMA_SRGB;

// One call of smvs_host_reconstruct_scene_*: what smvs_host_reconstruct_scene
// takes, then what the later entries added, each with the value the entries
// before it run with.
struct SceneCall
{
    const char *scene_dir;
    const smvs_host_recon_settings *o;
    const int *view_ids;
    int n_view_ids;
    int *reconstructed_out;
    int max_reconstructed;
    int *n_reconstructed, *n_skipped;
    double *seconds;
    int *input_scale_used;
    unsigned flags = 0u;
    SgmArgs sgm;
    unsigned known_flags = SCENE_FLAGS_REFINE;
};

int
reconstruct_scene_call(SceneCall const& c)
{
    return guarded([&] {
        SgmArgs const& a = c.sgm;
        check_sgm_records(a, "smvs_host_reconstruct_scene");
        require(!(a.sweep_on() && a.consensus != 0), "smvs_host_reconstruct_scene_sweep: "
            "sgm_sweep and sgm_consensus exclude each other");
        require(a.num_neighbors >= 1 && a.num_neighbors <= SMVS_MAX_SUBS
            && (a.consensus != 0 || a.sweep_on() || a.num_neighbors <= 2),
            "smvs_host_reconstruct_scene_merge: sgm_neighbors "
            "must be 1 or 2, or up to 16 with sgm_consensus or sgm_sweep");
        if (a.sweep_on()) {
            smvs_host_sgm_sweep const& s = *a.sweep;
            require(s.min_views >= -1 && s.min_views != 0 && s.min_views <= SMVS_MAX_SUBS
                && s.best_k >= -1 && s.best_k <= SMVS_MAX_SUBS && s.support_cost >= 0
                && s.support_cost <= 254 && s.min_support >= -1
                && s.min_support <= SMVS_MAX_SUBS,
                "smvs_host_reconstruct_scene_sweep: sgm_sweep_min_views "
                "must be -1 or in [1, 16], sgm_sweep_best_k and sgm_sweep_min_support -1 or in "
                "[0, 16], sgm_sweep_support_cost in [0, 254]");
        }
        require(a.consensus == 0 || (a.agree_ratio >= 0.0f && a.agree_ratio <= 1.0f
            && a.min_agree >= 1 && a.min_agree <= SMVS_MAX_SUBS),
            "smvs_host_reconstruct_scene_merge: sgm_agree_ratio "
            "must be in [0, 1] and sgm_min_agree in [1, 16]");
        require(SGMStereo::Options::valid_num_steps(a.num_steps),
            "smvs_host_reconstruct_scene_steps: sgm_num_steps "
            "must be in [2, 128] or a multiple of 8 in [136, 256]");
        require(c.scene_dir != nullptr && c.o != nullptr,
            "smvs_host_reconstruct_scene: bad argument");
        require((c.flags & ~c.known_flags) == 0u,
            "smvs_host_reconstruct_scene_flags: unknown flag");
        auto const flag = [&](unsigned bit) { return (c.flags & bit) != 0u; };
        require(!flag(SMVS_HOST_SCENE_INIT_SLANTS) || (a.refine != nullptr
            && a.refine->sweeps != 0), "smvs_host_reconstruct_scene_refine: init_slants needs "
            "sgm_refine_sweeps > 0");
        smvs_host_recon_settings const& o = *c.o;
        ReconSettings conf;
        if (o.image_embedding != nullptr)
            conf.image_embedding = o.image_embedding;
        conf.regularization = o.regularization;
        conf.output_scale = o.output_scale;
        conf.use_shading = o.use_shading != 0;
        conf.use_sgm = o.use_sgm != 0;
        conf.force_recon = o.force_recon != 0;
        conf.force_sgm = o.force_sgm != 0;
        conf.full_optimization = o.full_optimization != 0;
        conf.sgm = sgm_options(a, flag(SMVS_HOST_SCENE_ADAPTIVE_PENALTY2));
        conf.sgm.min_depth = o.sgm_min;
        conf.sgm.max_depth = o.sgm_max;
        conf.sgm.scale = o.sgm_scale;
        conf.device_input_scaling = flag(SMVS_HOST_SCENE_DEVICE_INPUT_SCALING);
        conf.device_shading_prep = flag(SMVS_HOST_SCENE_DEVICE_SHADING_PREP);
        conf.gamma_correction = flag(SMVS_HOST_SCENE_GAMMA_SRGB);
        conf.init_slants = flag(SMVS_HOST_SCENE_INIT_SLANTS);
        conf.num_neighbors = (std::size_t)o.num_neighbors;
        conf.min_neighbors = (std::size_t)o.min_neighbors;
        conf.first_device = o.first_device;
        conf.num_devices = o.num_devices;
        conf.views_in_flight = o.views_in_flight;
        conf.input_scale = o.input_scale;
        if (o.max_pixels > 0)
            conf.max_pixels = (std::size_t)o.max_pixels;
        if (c.view_ids != nullptr)
            conf.view_ids.assign(c.view_ids, c.view_ids + c.n_view_ids);
        ReconReport const report = reconstruct_scene(c.scene_dir, conf);
        if (c.reconstructed_out != nullptr && c.max_reconstructed > 0)
            std::copy_n(report.reconstructed.begin(),
                std::min<std::size_t>(report.reconstructed.size(),
                    (std::size_t)c.max_reconstructed), c.reconstructed_out);
        if (c.n_reconstructed != nullptr)
            *c.n_reconstructed = (int)report.reconstructed.size();
        if (c.n_skipped != nullptr)
            *c.n_skipped = (int)(report.skipped_few_neighbors.size()
                + report.already_done.size());
        if (c.seconds != nullptr)
            *c.seconds = report.seconds;
        if (c.input_scale_used != nullptr)
            *c.input_scale_used = report.input_scale;
    });
}

} // namespace

extern "C" int
smvs_host_reconstruct_scene(const char *scene_dir,
    const smvs_host_recon_settings *o, const int *view_ids, int n_view_ids,
    int *reconstructed_out, int max_reconstructed, int *n_reconstructed,
    int *n_skipped, double *seconds, int *input_scale_used)
{
    return reconstruct_scene_call({ scene_dir, o, view_ids, n_view_ids, reconstructed_out,
        max_reconstructed, n_reconstructed, n_skipped, seconds, input_scale_used });
}

extern "C" int
smvs_host_reconstruct_scene_mode(const char *scene_dir,
    const smvs_host_recon_settings *o, int sgm_adaptive_penalty2, const int *view_ids,
    int n_view_ids, int *reconstructed_out, int max_reconstructed, int *n_reconstructed,
    int *n_skipped, double *seconds, int *input_scale_used)
{
    return reconstruct_scene_call({ scene_dir, o, view_ids, n_view_ids, reconstructed_out,
        max_reconstructed, n_reconstructed, n_skipped, seconds, input_scale_used,
        sgm_adaptive_penalty2 != 0 ? SMVS_HOST_SCENE_ADAPTIVE_PENALTY2 : 0u });
}

extern "C" int
smvs_host_reconstruct_scene_flags(const char *scene_dir,
    const smvs_host_recon_settings *o, unsigned flags, const int *view_ids,
    int n_view_ids, int *reconstructed_out, int max_reconstructed, int *n_reconstructed,
    int *n_skipped, double *seconds, int *input_scale_used)
{
    return reconstruct_scene_call({ scene_dir, o, view_ids, n_view_ids, reconstructed_out,
        max_reconstructed, n_reconstructed, n_skipped, seconds, input_scale_used, flags });
}

extern "C" int
smvs_host_reconstruct_scene_steps(const char *scene_dir,
    const smvs_host_recon_settings *o, unsigned flags, int sgm_num_steps,
    const int *view_ids, int n_view_ids, int *reconstructed_out, int max_reconstructed,
    int *n_reconstructed, int *n_skipped, double *seconds, int *input_scale_used)
{
    return reconstruct_scene_call({ scene_dir, o, view_ids, n_view_ids, reconstructed_out,
        max_reconstructed, n_reconstructed, n_skipped, seconds, input_scale_used, flags,
        { sgm_num_steps } });
}

extern "C" int
smvs_host_reconstruct_scene_subplane(const char *scene_dir,
    const smvs_host_recon_settings *o, unsigned flags, int sgm_num_steps,
    int sgm_subplane, const int *view_ids, int n_view_ids, int *reconstructed_out,
    int max_reconstructed, int *n_reconstructed, int *n_skipped, double *seconds,
    int *input_scale_used)
{
    return reconstruct_scene_call({ scene_dir, o, view_ids, n_view_ids, reconstructed_out,
        max_reconstructed, n_reconstructed, n_skipped, seconds, input_scale_used, flags,
        { sgm_num_steps, sgm_subplane } });
}

extern "C" int
smvs_host_reconstruct_scene_merge(const char *scene_dir,
    const smvs_host_recon_settings *o, unsigned flags, int sgm_num_steps,
    int sgm_subplane, int sgm_neighbors, int sgm_consensus, float sgm_agree_ratio,
    int sgm_min_agree, const int *view_ids, int n_view_ids, int *reconstructed_out,
    int max_reconstructed, int *n_reconstructed, int *n_skipped, double *seconds,
    int *input_scale_used)
{
    return reconstruct_scene_call({ scene_dir, o, view_ids, n_view_ids, reconstructed_out,
        max_reconstructed, n_reconstructed, n_skipped, seconds, input_scale_used, flags,
        { sgm_num_steps, sgm_subplane, sgm_neighbors, sgm_consensus, sgm_agree_ratio,
            sgm_min_agree } });
}

extern "C" int
smvs_host_reconstruct_scene_sweep(const char *scene_dir,
    const smvs_host_recon_settings *o, unsigned flags, int sgm_num_steps,
    int sgm_subplane, int sgm_neighbors, int sgm_consensus, float sgm_agree_ratio,
    int sgm_min_agree, const smvs_host_sgm_sweep *sweep, const int *view_ids,
    int n_view_ids, int *reconstructed_out, int max_reconstructed, int *n_reconstructed,
    int *n_skipped, double *seconds, int *input_scale_used)
{
    return reconstruct_scene_call({ scene_dir, o, view_ids, n_view_ids, reconstructed_out,
        max_reconstructed, n_reconstructed, n_skipped, seconds, input_scale_used, flags,
        { sgm_num_steps, sgm_subplane, sgm_neighbors, sgm_consensus, sgm_agree_ratio,
            sgm_min_agree, sweep } });
}

extern "C" int
smvs_host_reconstruct_scene_filtered(const char *scene_dir,
    const smvs_host_recon_settings *o, unsigned flags, int sgm_num_steps,
    int sgm_subplane, int sgm_neighbors, int sgm_consensus, float sgm_agree_ratio,
    int sgm_min_agree, const smvs_host_sgm_sweep *sweep, const smvs_host_sgm_filter *filter,
    const int *view_ids, int n_view_ids, int *reconstructed_out, int max_reconstructed,
    int *n_reconstructed, int *n_skipped, double *seconds, int *input_scale_used)
{
    return reconstruct_scene_call({ scene_dir, o, view_ids, n_view_ids, reconstructed_out,
        max_reconstructed, n_reconstructed, n_skipped, seconds, input_scale_used, flags,
        { sgm_num_steps, sgm_subplane, sgm_neighbors, sgm_consensus, sgm_agree_ratio,
            sgm_min_agree, sweep, filter } });
}

extern "C" int
smvs_host_reconstruct_scene_photo(const char *scene_dir,
    const smvs_host_recon_settings *o, unsigned flags, int sgm_num_steps,
    int sgm_subplane, int sgm_neighbors, int sgm_consensus, float sgm_agree_ratio,
    int sgm_min_agree, const smvs_host_sgm_sweep *sweep, const smvs_host_sgm_filter *filter,
    const smvs_host_sgm_photo *photo, const int *view_ids, int n_view_ids,
    int *reconstructed_out, int max_reconstructed, int *n_reconstructed, int *n_skipped,
    double *seconds, int *input_scale_used)
{
    return reconstruct_scene_call({ scene_dir, o, view_ids, n_view_ids, reconstructed_out,
        max_reconstructed, n_reconstructed, n_skipped, seconds, input_scale_used, flags,
        { sgm_num_steps, sgm_subplane, sgm_neighbors, sgm_consensus, sgm_agree_ratio,
            sgm_min_agree, sweep, filter, photo } });
}

extern "C" int
smvs_host_reconstruct_scene_refine(const char *scene_dir,
    const smvs_host_recon_settings *o, unsigned flags, int sgm_num_steps,
    int sgm_subplane, int sgm_neighbors, int sgm_consensus, float sgm_agree_ratio,
    int sgm_min_agree, const smvs_host_sgm_sweep *sweep, const smvs_host_sgm_filter *filter,
    const smvs_host_sgm_photo *photo, const smvs_host_sgm_refine *refine, const int *view_ids,
    int n_view_ids, int *reconstructed_out, int max_reconstructed, int *n_reconstructed,
    int *n_skipped, double *seconds, int *input_scale_used)
{
    return reconstruct_scene_call({ scene_dir, o, view_ids, n_view_ids, reconstructed_out,
        max_reconstructed, n_reconstructed, n_skipped, seconds, input_scale_used, flags,
        { sgm_num_steps, sgm_subplane, sgm_neighbors, sgm_consensus, sgm_agree_ratio,
            sgm_min_agree, sweep, filter, photo, refine } });
}

extern "C" int
smvs_host_reconstruct_scene_planes(const char *scene_dir,
    const smvs_host_recon_settings *o, unsigned flags, int sgm_num_steps,
    int sgm_subplane, int sgm_neighbors, int sgm_consensus, float sgm_agree_ratio,
    int sgm_min_agree, const smvs_host_sgm_sweep *sweep, const smvs_host_sgm_filter *filter,
    const smvs_host_sgm_photo *photo, const smvs_host_sgm_refine *refine, const int *view_ids,
    int n_view_ids, int *reconstructed_out, int max_reconstructed, int *n_reconstructed,
    int *n_skipped, double *seconds, int *input_scale_used)
{
    return reconstruct_scene_call({ scene_dir, o, view_ids, n_view_ids, reconstructed_out,
        max_reconstructed, n_reconstructed, n_skipped, seconds, input_scale_used, flags,
        { sgm_num_steps, sgm_subplane, sgm_neighbors, sgm_consensus, sgm_agree_ratio,
            sgm_min_agree, sweep, filter, photo, refine },
        SCENE_FLAGS_REFINE | SMVS_HOST_SCENE_INIT_SLANTS });
}

extern "C" int
smvs_host_scene_info(const char *scene_dir, const char *image_embedding,
    int max_views, int *n_views, int *present, float *flen, float *rot9,
    float *trans3, int *width, int *height, int *n_features)
{
    return guarded([&] {
        require(scene_dir != nullptr && image_embedding != nullptr && n_views != nullptr,
            "smvs_host_scene_info: bad argument");
        Scene::Ptr scene = Scene::create(scene_dir);
        std::vector<SceneView> const& views = scene->get_views();
        *n_views = (int)views.size();
        require((int)views.size() <= max_views, "smvs_host_scene_info: more views than room");
        for (std::size_t i = 0; i < views.size(); ++i) {
            SceneView const& v = views[i];
            present[i] = v.present ? 1 : 0;
            flen[i] = v.camera.flen;
            std::copy(v.camera.rot, v.camera.rot + 9, rot9 + 9 * i);
            std::copy(v.camera.trans, v.camera.trans + 3, trans3 + 3 * i);
            int whc[3] = { 0, 0, 0 };
            if (v.present && v.has_image(image_embedding))
                (void)v.image_size(image_embedding, whc);
            width[i] = whc[0];
            height[i] = whc[1];
        }
        if (n_features != nullptr) {
            try {
                *n_features = (int)scene->get_bundle()->features.size();
            } catch (std::exception const&) {
                *n_features = -1;
            }
        }
    });
}

extern "C" int
smvs_host_select_neighbors(const smvs_host_view *views_in, int n_views,
    const smvs_host_bundle *bundle_in, int view, int num_neighbors, int *out,
    int *n_out)
{
    return guarded([&] {
        require(views_in != nullptr && out != nullptr && n_out != nullptr
            && view >= 0 && view < n_views && num_neighbors >= 0,
            "smvs_host_select_neighbors: bad argument");
        ViewSelection::ViewList views((std::size_t)n_views);
        for (int i = 0; i < n_views; ++i) {
            smvs_host_view const& v = views_in[i];
            ViewSelection::ViewInfo& info = views[i];
            info.present = v.width > 0;
            info.id = v.view_id;
            info.cam = make_camera(v);
            info.has_image = v.bytes != nullptr;
            info.width = v.width;
            info.height = v.height;
        }
        ViewSelection::Options opts;
        opts.num_neighbors = (std::size_t)num_neighbors;
        ViewSelection selection(opts, views, make_bundle(bundle_in));
        std::vector<std::size_t> const chosen
            = selection.get_neighbors_for_view((std::size_t)view);
        *n_out = (int)chosen.size();
        for (std::size_t k = 0; k < chosen.size(); ++k)
            out[k] = (int)chosen[k];
    });
}

extern "C" int
smvs_host_mvei_roundtrip(const char *in_path, const char *out_path)
{
    return guarded([&] {
        require(in_path != nullptr && out_path != nullptr,
            "smvs_host_mvei_roundtrip: bad argument");
        int whct[4];
        if (!mvei_header(in_path, whct))
            throw std::runtime_error(std::string("not an .mvei file: ") + in_path);
        if (whct[3] == 1)
            save_mvei(out_path, ByteImage::ConstPtr(load_mvei_u8(in_path)));
        else
            save_mvei(out_path, FloatImage::ConstPtr(load_mvei_float(in_path)));
    });
}

extern "C" int
smvs_host_load_byte_image(const char *path, int *whc, uint8_t *pixels, size_t capacity)
{
    return guarded([&] {
        require(path != nullptr && whc != nullptr, "smvs_host_load_byte_image: bad argument");
        std::string const p = path;
        auto ends_with = [&](char const* ext) {
            std::size_t const n = std::strlen(ext);
            return p.size() > n && p.compare(p.size() - n, n, ext) == 0;
        };
        ByteImage::Ptr img = ends_with(".png") ? load_png_u8(p)
            : (ends_with(".jpg") || ends_with(".jpeg")) ? load_jpeg_u8(p) : load_mvei_u8(p);
        whc[0] = img->width();
        whc[1] = img->height();
        whc[2] = img->channels();
        std::size_t const n = (std::size_t)img->width() * img->height() * img->channels();
        if (pixels != nullptr) {
            require(capacity >= n, "smvs_host_load_byte_image: buffer too small");
            std::memcpy(pixels, img->begin(), n);
        }
    });
}

extern "C" int
smvs_host_save_png(const char *path, const uint8_t *pixels, int width, int height,
    int channels)
{
    return guarded([&] {
        require(path != nullptr && pixels != nullptr && width >= 1 && height >= 1,
            "smvs_host_save_png: bad argument");
        save_png_u8(path, byte_image_from(pixels, width, height, channels));
    });
}

extern "C" int
smvs_host_rescale_half_size_gaussian(const uint8_t *pixels, int width, int height,
    int channels, uint8_t *out)
{
    return guarded([&] {
        require(pixels != nullptr && out != nullptr && channels >= 1,
            "smvs_host_rescale_half_size_gaussian: bad argument");
        ByteImage::Ptr half = rescale_half_size_gaussian(byte_image_from(pixels, width, height,
            channels));
        std::memcpy(out, half->begin(),
            (std::size_t)half->width() * half->height() * half->channels());
    });
}

extern "C" int
smvs_host_rescale_half_size_gaussian_device(const uint8_t *pixels, int width, int height,
    int channels, int halvings, int device, uint8_t *out, size_t out_capacity,
    int *out_width, int *out_height)
{
    return guarded([&] {
        require(pixels != nullptr && out != nullptr && out_width != nullptr
            && out_height != nullptr && width >= 1 && height >= 1 && channels >= 1,
            "smvs_host_rescale_half_size_gaussian_device: bad argument");
        ByteImage::Ptr scaled = rescale_half_size_gaussian_device(byte_image_from(pixels, width,
            height, channels), halvings, device);
        std::size_t const n = (std::size_t)scaled->width() * scaled->height()
            * scaled->channels();
        require(out_capacity >= n,
            "smvs_host_rescale_half_size_gaussian_device: buffer too small");
        std::memcpy(out, scaled->begin(), n);
        *out_width = scaled->width();
        *out_height = scaled->height();
    });
}
