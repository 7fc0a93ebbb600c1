// Per-patch topology tests of DepthOptimizer between Newton batches
// (SURVEY.md row (f)-2), on the device:
//
//   * create_subview_surfaces (lib/depth_optimizer.cc:433-604): z-buffer of
//     the current surface (and of the SGM depth) in every neighbour, then per
//     (patch, neighbour) the image-border / occlusion test, the warp
//     anisotropy test and ncc_for_patch (:792-912) -> visibility bit mask;
//   * mse_for_patch (:747-790) for every valid patch, the quantity
//     cut_boundaries (:360-431) thresholds.
//
// The host keeps the topology itself (which patches and nodes exist): these
// kernels only produce the per-patch numbers the host decides on, and they do
// so with the arithmetic of csrc/host/topo_math.h (the source the C++ host
// mirror compiles too).  The z-buffer minimum is order independent:
// (float)min(d) == min((float)d) because rounding is monotone.
//
// This file: the argument block of all kernels and the entry point of the
// visibility masks.  The kernels, each with the host function that launches
// it: topo_zbuffer.hip, topo_visibility.hip (its launch shape:
// topo_vis_plan.h), topo_mse.hip (smvs_topology_patch_mse), topo_cut.hip
// (smvs_topology_cut_boundaries); shared: topo_internal.h, topo_divide.h.
#include "topo_internal.h"

#include <cstdlib>
#include <cstring>
#include <vector>

namespace smvs_hip {

int
fill_args(smvs_ctx *ctx, TopoArgs *A, const char *who)
{
    if (!ctx->has_surface || !ctx->has_cameras) {
        set_error("%s: cameras and surface must be set first", who);
        return SMVS_ERR_STATE;
    }
    for (int v = 0; v <= ctx->n_subs; ++v)
        if (!((ctx->image_ok >> v) & 1u)) {
            set_error("%s: view %d has no image (smvs_ctx_upload_image)", who,
                v - 1);
            return SMVS_ERR_STATE;
        }
    {
        // (images handed over by smvs_ctx_upload_image_async and not read yet)
        int const rc = ctx_materialise_images(ctx, ~0u);
        if (rc != SMVS_OK)
            return rc;
    }
    A->nodes = ctx->nodes;
    A->patch_valid = ctx->patch_valid;
    A->patch_vis = ctx->patch_vis;
    A->vis_out = ctx->patch_vis;
    A->mse_out = ctx->topo_mse;
    A->cams = ctx->cams;
    for (int v = 0; v <= ctx->n_subs; ++v) {
        A->views[v].w = ctx->images[v].w;
        A->views[v].h = ctx->images[v].h;
        A->views[v].c = ctx->images[v].c;
        A->views[v].image = ctx->images[v].data;
    }
    A->main_grad = ctx->main_grad;
    A->subs = ctx->subs_dev;
    for (int s = 0; s < SMVS_MAX_SUBS; ++s) {
        A->zbuf[s] = ctx->topo_zbuf[s];
        A->zraw[s] = ctx->topo_zbuf[s] == nullptr ? nullptr
            : ctx->topo_zbuf[s] + (size_t)(ctx->images[1 + s].w + 1)
                * (ctx->images[1 + s].h + 1);
    }
    A->sgm_depth = nullptr;
    {
        const char *mode = std::getenv("SMVS_TOPO_DIVIDE");
        A->exact_divisions = mode != nullptr && std::strcmp(mode, "exact") == 0 ? 1 : 0;
        const char *pairs = std::getenv("SMVS_NCC_PAIRS");
        A->ncc_pairs = pairs != nullptr && std::atoi(pairs) == 0 ? 0 : 1;
        const char *window = std::getenv("SMVS_ZBUF_WINDOW");
        A->zbuf5 = window != nullptr && std::atoi(window) == 3 ? 0 : 1;
    }

    A->ncc = ctx->topo_ncc;
    for (int i = 0; i < 33; ++i)
        A->ncc_off[i] = ctx->topo_ncc_off[i];
    A->W = ctx->width;
    A->H = ctx->height;
    A->npx = ctx->npx;
    A->npy = ctx->npy;
    A->stride = ctx->node_stride;
    A->ps = ctx->patchsize;
    A->ps_log2 = 0;
    while ((1 << A->ps_log2) < ctx->patchsize)
        A->ps_log2 += 1;
    A->inv_ps = 1.0 / (double)ctx->patchsize;
    A->start_x = ctx->start_x;
    A->start_y = ctx->start_y;
    A->n_subs = ctx->n_subs;
    A->num_patches = ctx->num_patches;
    A->use_ncc = 0;
    A->patch_valid_rw = ctx->patch_valid;
    A->node_valid_rw = ctx->node_valid;
    A->deleted = ctx->status + I_TOPO_DELETED;
    A->mse_list = ctx->topo_mse_list;
    A->mse_count = ctx->status + I_TOPO_CANDIDATES;
    A->num_nodes = ctx->num_nodes;
    A->border_node = ctx->topo_border;
    A->only_candidates = 0;
    A->pix = ctx->topo_pix;
    for (int i = 0; i < 9; ++i)
        A->invproj[i] = 0.0f;
    return SMVS_OK;
}

} // namespace smvs_hip

using namespace smvs_hip;

extern "C" int
smvs_topology_subviews(smvs_ctx *ctx, const float *sgm_depth, int use_ncc,
    uint32_t *patch_vis_out)
{
    SMVS_REQUIRE(ctx != nullptr, "null argument");
    SMVS_HIP_CHECK(set_device(ctx->device));
    if ((ctx->image_ok & 1u) != 0u
        && (ctx->images[0].w != ctx->width || ctx->images[0].h != ctx->height)) {
        set_error("smvs_topology_subviews: main image size differs from the context");
        return SMVS_ERR_INVALID;
    }
    // (the kernels index the per-pixel planes and the float images with 32-bit offsets)
    if ((size_t)ctx->width * ctx->height * 3 >= ((size_t)1 << 31)) {
        set_error("smvs_topology_subviews: images of 2^31 / 3 pixels and more are not supported");
        return SMVS_ERR_INVALID;
    }
    for (int j = 0; j <= ctx->n_subs; ++j)
        if ((size_t)ctx->images[j].w * ctx->images[j].h * 3 >= ((size_t)1 << 31)) {
            set_error("smvs_topology_subviews: images of 2^31 / 3 pixels and more are not supported");
            return SMVS_ERR_INVALID;
        }
    int rc;
    // the 32 sample templates of ncc_for_patch for this patch size
    if (ctx->topo_ncc_ps != ctx->patchsize && ctx->has_surface) {
        std::vector<smvs_topo::NccSample> all;
        for (int f = 0; f < 32; ++f) {
            ctx->topo_ncc_off[f] = (int)all.size();
            std::vector<smvs_topo::NccSample> const one
                = smvs_topo::build_ncc_template(ctx->patchsize, f);
            all.insert(all.end(), one.begin(), one.end());
        }
        ctx->topo_ncc_off[32] = (int)all.size();
        // (the old templates go first: no patch size says they are there until
        // the new ones are)
        ctx->topo_ncc_ps = 0;
        if ((rc = device_alloc(&ctx->topo_ncc, all.size())) != SMVS_OK)
            return rc;
        SMVS_HIP_CHECK(hipMemcpyAsync(ctx->topo_ncc, all.data(),
            all.size() * sizeof(smvs_topo::NccSample), hipMemcpyHostToDevice,
            ctx->stream));
        SMVS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        ctx->topo_ncc_ps = ctx->patchsize;
    }
    for (int s = 0; s < ctx->n_subs; ++s) {
        size_t const n = (size_t)(ctx->images[1 + s].w + 1)
            * (ctx->images[1 + s].h + 1);
        // (the z-buffer and, behind it, the per-centre minima: 2 * n floats, the
        // capacity counts the n cells of one)
        if ((rc = device_grow(&ctx->topo_zbuf[s], &ctx->topo_zbuf_cap[s], n, 2)) != SMVS_OK)
            return rc;
    }
    size_t const npix = (size_t)ctx->width * ctx->height;
    if ((rc = device_grow(&ctx->topo_pix, &ctx->topo_pix_cap, npix * 3)) != SMVS_OK)
        return rc;
    if (sgm_depth != nullptr
        && (rc = device_grow(&ctx->topo_sgm, &ctx->topo_sgm_cap, npix)) != SMVS_OK)
        return rc;
    TopoArgs A;
    if ((rc = fill_args(ctx, &A, "smvs_topology_subviews")) != SMVS_OK)
        return rc;
    A.use_ncc = use_ncc ? 1 : 0;
    if (sgm_depth != nullptr) {
        if ((rc = ctx_upload(ctx, ctx->topo_sgm, sgm_depth, npix * sizeof(float)))
                != SMVS_OK)
            return rc;
        ctx->sgm_resident = false;   // (overwritten by the caller's map)
        A.sgm_depth = ctx->topo_sgm;
    } else if (ctx->sgm_resident) {
        // the map smvs_ctx_sgm_init_depth left on the device
        A.sgm_depth = ctx->topo_sgm;
    }
    launch_zbuffers(ctx, A);
    if ((rc = launch_visibility(ctx, &A)) != SMVS_OK)
        return rc;
    if (patch_vis_out == nullptr)
        return SMVS_OK;   // (the masks stay on the device: surface.hip)
    SMVS_HIP_CHECK(hipMemcpyAsync(patch_vis_out, ctx->patch_vis,
        sizeof(uint32_t) * ctx->num_patches, hipMemcpyDeviceToHost,
        ctx->stream));
    SMVS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return SMVS_OK;
}
