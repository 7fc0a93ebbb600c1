// C ABI of the host mirror (host_capi.h): smvs::Surface on its own, on the host
// and on a device context, and the maps of a surface without optimize().
#include "capi_internal.h"

#include "depth_optimizer.h"
#include "surface.h"

using namespace smvs_amd;
using namespace smvs_amd::capi;

namespace {

// what the three `_planes` entries ask before they share a body
int
require_planes(const float *init_depth, const float *init_slant, std::string const& entry)
{
    return guarded([&] {
        require(init_depth != nullptr && init_slant != nullptr,
            entry + ": init_depth and init_slant are required");
    });
}

int
surface_script(const smvs_host_view *main_in,
    const smvs_host_bundle *bundle_in, const float *init_depth, const float *init_slant,
    int init_scale, const int *ops, int n_ops, int delete_every, int *info, double *nodes_out,
    uint8_t *node_valid_out, uint8_t *patch_valid_out)
{
    return guarded([&] {
        require(main_in != nullptr && info != nullptr && nodes_out != nullptr
            && node_valid_out != nullptr && patch_valid_out != nullptr
            && (n_ops <= 0 || ops != nullptr) && delete_every >= 1,
            "smvs_host_surface_script: bad argument");
        StereoView::Ptr main_view = make_view(*main_in);
        Surface::Ptr surface = Surface::create(make_bundle(bundle_in), main_view, init_scale,
            float_image_from(init_depth, main_in->width, main_in->height, 1),
            float_image_from(init_slant, main_in->width, main_in->height, 2));
        for (int k = 0; k < n_ops; ++k)
            switch (ops[k]) {
            case 1: surface->expand(); break;
            case 2: surface->subdivide_patches(); break;
            case 3: surface->fill_patches_from_depth(); break;
            case 4: surface->remove_isolated_patches(); break;
            case 5: {
                int seen = 0;
                for (std::size_t p = 0; p < surface->patch_validity().size(); ++p)
                    if (surface->patch_validity()[p] && (++seen % delete_every) == 0)
                        surface->delete_patch(p);
                surface->remove_nodes_without_patch();
                break;
            }
            default:
                throw std::invalid_argument("smvs_host_surface_script: unknown operation");
            }
        Surface const& s = *surface;
        info[0] = s.get_scale();
        info[1] = s.get_num_patches_x();
        info[2] = s.get_num_patches_y();
        info[3] = s.get_pixel_start_x();
        info[4] = s.get_pixel_start_y();
        std::copy(s.node_values().begin(), s.node_values().end(), nodes_out);
        std::copy(s.node_validity().begin(), s.node_validity().end(), node_valid_out);
        std::copy(s.patch_validity().begin(), s.patch_validity().end(), patch_valid_out);
    });
}

// a device context that ends with its scope, on either exit
struct Context
{
    smvs_ctx *ctx = nullptr;
    Context() = default;
    Context(Context const&) = delete;
    Context& operator=(Context const&) = delete;
    ~Context() { if (ctx != nullptr) smvs_ctx_destroy(ctx); }
};

// The same script on the surface of a device context (csrc/surface.hip).
int
surface_script_device(const smvs_host_view *main_in,
    const smvs_host_bundle *bundle_in, const float *init_depth, const float *init_slant,
    int init_scale, const int *ops, int n_ops, int delete_every, int device, int *info,
    double *nodes_out, uint8_t *node_valid_out, uint8_t *patch_valid_out)
{
    return guarded([&] {
        require(main_in != nullptr && info != nullptr && nodes_out != nullptr
            && node_valid_out != nullptr && patch_valid_out != nullptr
            && (n_ops <= 0 || ops != nullptr) && delete_every >= 1,
            "smvs_host_surface_script_device: bad argument");
        auto check = [](int rc, char const* what) {
            if (rc != SMVS_OK)
                throw std::runtime_error(std::string(what) + ": " + smvs_last_error());
        };
        StereoView::Ptr main_view = make_view(*main_in);
        Context c;
        check(smvs_ctx_create(device, main_in->width, main_in->height, 1, &c.ctx),
            "smvs_ctx_create");
        smvs_ctx *const ctx = c.ctx;
        int valid = 0;
        if (init_slant != nullptr) {
            check(smvs_surface_create_planes(ctx, init_scale, init_depth, init_slant, &valid),
                "smvs_surface_create_planes");
        } else if (init_depth != nullptr) {
            check(smvs_surface_create(ctx, init_scale, init_depth, nullptr, nullptr, 0,
                &valid), "smvs_surface_create");
        } else {
            Bundle::Ptr bundle = make_bundle(bundle_in);
            std::vector<int32_t> pixels;
            std::vector<float> depths;
            Surface::project_bundle(bundle, main_view->get_camera(),
                main_view->get_view_id(), main_in->width, main_in->height, &pixels,
                &depths);
            require(!pixels.empty(), "smvs_host_surface_script_device: the "
                "bundle has no feature in this view");
            check(smvs_surface_create(ctx, init_scale, nullptr, pixels.data(),
                depths.data(), (int)pixels.size(), &valid), "smvs_surface_create");
        }
        for (int k = 0; k < n_ops; ++k)
            switch (ops[k]) {
            case 1: check(smvs_surface_expand(ctx, nullptr, &valid), "expand"); break;
            case 2: check(smvs_surface_subdivide(ctx, &valid), "subdivide"); break;
            case 3: check(smvs_surface_fill_patches_from_depth(ctx, &valid), "fill"); break;
            case 4: check(smvs_surface_remove_isolated_patches(ctx, &valid), "isolated"); break;
            case 5: check(smvs_surface_delete_every(ctx, delete_every, &valid), "delete"); break;
            default:
                throw std::invalid_argument("smvs_host_surface_script_device: unknown operation");
            }
        smvs_surface_geometry g;
        int counted = 0;
        check(smvs_surface_info(ctx, &g, &counted), "smvs_surface_info");
        if (counted != valid)
            throw std::runtime_error("smvs_host_surface_script_device: the operation's "
                "count of valid patches differs from a recount");
        info[0] = g.scale;
        info[1] = g.npx;
        info[2] = g.npy;
        info[3] = g.start_x;
        info[4] = g.start_y;
        info[5] = valid;
        check(smvs_surface_download(ctx, nodes_out, node_valid_out, patch_valid_out,
            nullptr), "smvs_surface_download");
    });
}

int
surface_maps(const smvs_host_view *main_in, const smvs_host_view *subs_in,
    int n_subs, const smvs_host_bundle *bundle_in, const float *init_depth,
    const float *init_slant, int init_scale, int device, float *depth_out, float *normals_out)
{
    return guarded([&] {
        require(main_in != nullptr && subs_in != nullptr && n_subs >= 1
            && depth_out != nullptr && normals_out != nullptr,
            "smvs_host_surface_maps: bad argument");
        StereoView::Ptr main_view = make_view(*main_in);
        std::vector<StereoView::Ptr> subs = make_views(subs_in, n_subs);
        Surface::Ptr surface = Surface::create(make_bundle(bundle_in), main_view, init_scale,
            float_image_from(init_depth, main_in->width, main_in->height, 1),
            float_image_from(init_slant, main_in->width, main_in->height, 2));
        DepthOptimizer::Options opts;
        opts.device = device;
        // lib/depth_optimizer.h:53-61: the surface constructor, then the
        // maps without a prior optimize()
        DepthOptimizer optimizer(main_view, subs, surface, opts);
        std::size_t const npix = (std::size_t)main_in->width * main_in->height;
        std::memcpy(depth_out, optimizer.get_depth()->begin(), sizeof(float) * npix);
        std::memcpy(normals_out, optimizer.get_normals()->begin(),
            sizeof(float) * 3 * npix);
    });
}

} // namespace

extern "C" int
smvs_host_surface_script(const smvs_host_view *main_in,
    const smvs_host_bundle *bundle_in, const float *init_depth, int init_scale,
    const int *ops, int n_ops, int delete_every, int *info, double *nodes_out,
    uint8_t *node_valid_out, uint8_t *patch_valid_out)
{
    return surface_script(main_in, bundle_in, init_depth, nullptr, init_scale, ops, n_ops,
        delete_every, info, nodes_out, node_valid_out, patch_valid_out);
}

extern "C" int
smvs_host_surface_script_planes(const smvs_host_view *main_in, const float *init_depth,
    const float *init_slant, int init_scale, const int *ops, int n_ops, int delete_every,
    int *info, double *nodes_out, uint8_t *node_valid_out, uint8_t *patch_valid_out)
{
    int const status = require_planes(init_depth, init_slant, "smvs_host_surface_script_planes");
    return status != 0 ? status : surface_script(main_in, nullptr, init_depth, init_slant,
        init_scale, ops, n_ops, delete_every, info, nodes_out, node_valid_out, patch_valid_out);
}

extern "C" int
smvs_host_surface_script_device(const smvs_host_view *main_in,
    const smvs_host_bundle *bundle_in, const float *init_depth, int init_scale,
    const int *ops, int n_ops, int delete_every, int device, int *info,
    double *nodes_out, uint8_t *node_valid_out, uint8_t *patch_valid_out)
{
    return surface_script_device(main_in, bundle_in, init_depth, nullptr, init_scale, ops,
        n_ops, delete_every, device, info, nodes_out, node_valid_out, patch_valid_out);
}

extern "C" int
smvs_host_surface_script_planes_device(const smvs_host_view *main_in, const float *init_depth,
    const float *init_slant, int init_scale, const int *ops, int n_ops, int delete_every,
    int device, int *info, double *nodes_out, uint8_t *node_valid_out,
    uint8_t *patch_valid_out)
{
    int const status = require_planes(init_depth, init_slant,
        "smvs_host_surface_script_planes_device");
    return status != 0 ? status : surface_script_device(main_in, nullptr, init_depth,
        init_slant, init_scale, ops, n_ops, delete_every, device, info, nodes_out,
        node_valid_out, patch_valid_out);
}

extern "C" int
smvs_host_slant_plane(const float *lowres, const float *slants, int dm_w, int dm_h, int width,
    int height, float *out)
{
    return guarded([&] {
        require(lowres != nullptr && slants != nullptr && out != nullptr && dm_w >= 1
            && dm_h >= 1 && width >= 1 && height >= 1, "smvs_host_slant_plane: bad argument");
        FloatImage::Ptr p = Surface::slant_plane(float_image_from(lowres, dm_w, dm_h, 1),
            float_image_from(slants, dm_w, dm_h, 2), width, height);
        std::memcpy(out, p->begin(), sizeof(float) * 2 * (std::size_t)width * height);
    });
}

extern "C" int
smvs_host_surface_maps(const smvs_host_view *main_in, const smvs_host_view *subs_in,
    int n_subs, const smvs_host_bundle *bundle_in, const float *init_depth,
    int init_scale, int device, float *depth_out, float *normals_out)
{
    return surface_maps(main_in, subs_in, n_subs, bundle_in, init_depth, nullptr, init_scale,
        device, depth_out, normals_out);
}

extern "C" int
smvs_host_surface_maps_planes(const smvs_host_view *main_in, const smvs_host_view *subs_in,
    int n_subs, const smvs_host_bundle *bundle_in, const float *init_depth,
    const float *init_slant, int init_scale, int device, float *depth_out, float *normals_out)
{
    int const status = require_planes(init_depth, init_slant, "smvs_host_surface_maps_planes");
    return status != 0 ? status : surface_maps(main_in, subs_in, n_subs, bundle_in, init_depth,
        init_slant, init_scale, device, depth_out, normals_out);
}

extern "C" int
smvs_host_surface_maps_host(const smvs_host_view *main_in, const float *init_depth,
    const float *init_slant, int init_scale, float *depth_out, float *normals_out)
{
    return guarded([&] {
        require(main_in != nullptr && init_depth != nullptr,
            "smvs_host_surface_maps_host: bad argument");
        StereoView::Ptr main_view = make_view(*main_in);
        Surface::Ptr surface = Surface::create(nullptr, main_view, init_scale,
            float_image_from(init_depth, main_in->width, main_in->height, 1),
            float_image_from(init_slant, main_in->width, main_in->height, 2));
        std::size_t const npix = (std::size_t)main_in->width * main_in->height;
        if (depth_out != nullptr)
            std::memcpy(depth_out, surface->get_depth_map()->begin(), sizeof(float) * npix);
        if (normals_out != nullptr)
            std::memcpy(normals_out,
                surface->get_normal_map(main_view->get_inverse_flen())->begin(),
                sizeof(float) * 3 * npix);
    });
}
