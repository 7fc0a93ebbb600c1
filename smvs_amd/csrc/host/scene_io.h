// MVE scene I/O for the host mirror and the scene-level driver of smvsrecon
// (reference: app/smvsrecon.cc:388-752; mve::Scene / mve::View / mve::Bundle
// are MVE's, not in the reference tree: every format detail below is
// [MVE-unverified] and listed in tests/golden/README.md).
//
// What is read: views/view_XXXX.mve/meta.ini ([camera] focal_length,
// pixel_aspect, principal_point, rotation, translation; [view] id, name), the
// bundle synth_0.out ("drews 1.0"), raw .mvei images (u8 / float) and PNG
// byte images (csrc/host/png_io.cc, on zlib) -- what makescene leaves in a
// view directory ("undistorted.png").  JPEG embeddings are not decoded (no
// codec in this tree; a view whose only copy of the embedding is a .jpg is
// reported with that reason).  Results are written like StereoView::
// write_depth_to_view / write_image_to_view do (lib/stereo_view.h:100-130):
// <output>.mvei (depth, MVE ray-length convention), <output>N.mvei (normals),
// smvs-sgm.mvei.
#pragma once

#include <string>
#include <vector>

#include "image.h"
#include "view_selection.h"

namespace smvs_amd {

// \211MVE_IMAGE\n + int32 width, height, channels, type + raw data
ByteImage::Ptr load_mvei_u8(std::string const& path);
FloatImage::Ptr load_mvei_float(std::string const& path);
void save_mvei(std::string const& path, ByteImage::ConstPtr image);
void save_mvei(std::string const& path, FloatImage::ConstPtr image);
// width, height, channels, type of an .mvei file without loading it
bool mvei_header(std::string const& path, int* whct);

struct SceneView
{
    bool present = false;        // a null View::Ptr otherwise
    int id = 0;
    std::string name, directory;
    CameraInfo camera;
    bool is_camera_valid(void) const { return camera.flen > 0.0f; }
    // mve::View::has_image: <embedding>.mvei or <embedding>.png (a .jpg alone
    // does not count: it cannot be decoded here)
    bool has_image(std::string const& embedding) const;
    // the file of an embedding: the existing .mvei, else the existing .png,
    // else where a NEW embedding of that name is written (.mvei)
    std::string image_path(std::string const& embedding) const;
    // byte image of an embedding (mve::View::get_byte_image), any container
    ByteImage::Ptr load_byte_image(std::string const& embedding) const;
    // width, height, channels without decoding (mve::View::get_image_proxy)
    bool image_size(std::string const& embedding, int* whc) const;
};

// mve::image::rescale_half_size_gaussian<uint8_t> (sigma^2 = 0.75), the filter
// smvsrecon pre-scales its input embedding with (app/smvsrecon.cc:634-647)
// [MVE-unverified, tests/golden/README.md M29]
ByteImage::Ptr rescale_half_size_gaussian(ByteImage::ConstPtr image);
// `halvings` of them chained on device `device` (smvs_rescale_half_gaussian),
// bit-identical with the host function applied `halvings` times; throws
// std::invalid_argument for what the device entry refuses (more than four
// channels, a level too small), std::runtime_error for a device error
ByteImage::Ptr rescale_half_size_gaussian_device(ByteImage::ConstPtr image,
    int halvings, int device);

class Scene
{
public:
    typedef std::shared_ptr<Scene> Ptr;
    // mve::Scene::create(path): views/view_*.mve, list index = view id
    static Ptr create(std::string const& path);
    std::vector<SceneView>& get_views(void) { return views; }
    // mve::Scene::get_bundle(): <path>/synth_0.out; throws if unreadable
    Bundle::Ptr get_bundle(void) const;
    std::string const& get_path(void) const { return path; }
private:
    std::string path;
    std::vector<SceneView> views;
};

Bundle::Ptr load_mve_bundle(std::string const& path);

// AppSettings of app/smvsrecon.cc:37-71 (the part that reaches the per-view task)
struct ReconSettings
{
    std::vector<int> view_ids;              // empty: every view with a valid camera
    std::string image_embedding = "undistorted";
    float regularization = 1.0f;            // alpha
    int output_scale = 2;                   // -o
    int input_scale = -1;                   // -s; < 0: automatic (:477-500)
    std::size_t max_pixels = 1700000;       // --max-pixels (:48)
    bool use_shading = false;               // -S
    float light_surf_regularization = 0.0f;
    bool gamma_correction = false;
    bool use_sgm = true;
    bool force_recon = false, force_sgm = false, full_optimization = false;
    float sgm_min = 0.0f, sgm_max = 0.0f;
    int sgm_scale = 1;
    // not in the reference's AppSettings: SGMStereo::Options::adaptive_penalty2
    // (the reference's build without SSE, lib/sgm_stereo.cc:310-346)
    bool sgm_adaptive_penalty2 = false;
    // not in the reference's AppSettings (app/smvsrecon.cc:693-709 leaves
    // SGMStereo::Options::num_steps at its default): the inverse-depth planes of
    // the SGM front end, 2 .. 128 or a multiple of 8 from 136 to 256
    int sgm_num_steps = 128;
    // not in the reference's AppSettings: SGMStereo::Options::subplane (the
    // smvs-sgm map refined between the planes).  An smvs-sgm embedding of the
    // right size is reused as before (app/smvsrecon.cc:702-708): switching this
    // on for a scene that has one needs force_sgm
    bool sgm_subplane = false;
    // not in the reference's AppSettings: SGMStereo::Options::num_neighbors /
    // consensus / agree_ratio / min_agree -- the smvs-sgm map of a view from its
    // first sgm_neighbors neighbours (capped by the neighbours the view has),
    // merged by consensus; more than two need sgm_consensus.  0.95 and 2 are
    // defaults of a user option, not tuned values, and their effect on real
    // scenes has not been measured.  As for sgm_subplane, an smvs-sgm embedding
    // of the right size is reused: switching this on for a scene that has one
    // needs force_sgm
    int sgm_neighbors = 2;
    bool sgm_consensus = false;
    float sgm_agree_ratio = 0.95f;
    int sgm_min_agree = 2;
    // SGMStereo::Options::sweep / sweep_min_views / sweep_best_k /
    // sweep_support_cost / sweep_min_support -- the smvs-sgm map of a view by the
    // plane sweep over its first sgm_neighbors neighbours (not together with
    // sgm_consensus); -1: the default at n neighbours.  Untuned defaults of a
    // user option; the reuse rule is that of sgm_subplane (force_sgm).
    bool sgm_sweep = false;
    int sgm_sweep_min_views = -1;
    int sgm_sweep_best_k = -1;
    int sgm_sweep_support_cost = 20;
    int sgm_sweep_min_support = -1;
    // SGMStereo::Options::uniqueness / uniqueness_window / speckle_size /
    // speckle_ratio -- the two filters of include/smvs_hip.h ("Two single-run
    // rejections") in every view's SGM front end, whichever of the three it is.
    // Off by default; untuned defaults of a user option; the reuse rule is that
    // of sgm_subplane (force_sgm).
    int sgm_uniqueness = 0;
    int sgm_uniqueness_window = 1;
    int sgm_speckle_size = 0;
    float sgm_speckle_ratio = 0.95f;
    // SGMStereo::Options::photo_radius / photo_best_k / photo_min_views /
    // photo_min_score / photo_witnesses -- the multi-view photo-consistency test
    // of include/smvs_hip.h behind every view's SGM front end, whichever of the
    // three it is, with the view's neighbours as witnesses (-1: all num_neighbors
    // of them); the confidence is saved as smvs-sgm-confidence next to smvs-sgm.
    // Off by default (radius 0); untuned defaults of a user option; the reuse
    // rule is that of sgm_subplane (force_sgm).
    int sgm_photo_radius = 0;
    int sgm_photo_best_k = 2;
    int sgm_photo_min_views = 2;
    float sgm_photo_min_score = 0.49f;
    int sgm_photo_witnesses = -1;
    // SGMStereo::Options::refine_sweeps / refine_samples / refine_depth_step /
    // refine_slant_step / refine_seed / refine_fill -- the multi-view plane
    // refinement sweeps of include/smvs_hip.h in the photo test's place (they
    // need sgm_photo_radius > 0); the slants are saved as smvs-sgm-slant (two
    // channels) next to smvs-sgm-confidence; the optimizer reads them with
    // init_slants only.  Off by default (sweeps 0); untuned defaults of a user option; the
    // reuse rule is that of sgm_subplane (force_sgm).
    int sgm_refine_sweeps = 0;
    int sgm_refine_samples = 2;
    float sgm_refine_depth_step = 0.02f;
    float sgm_refine_slant_step = 0.01f;
    uint32_t sgm_refine_seed = 1;
    int sgm_refine_fill = 1;
    // not in the reference's AppSettings: the input scaling of :621-650 on the
    // device (rescale_half_size_gaussian_device), one ViewQueue task per view
    bool device_input_scaling = false;
    // not in the reference's AppSettings: DepthOptimizer::Options::
    // device_shading_prep (with use_shading only)
    bool device_shading_prep = false;
    // not in the reference's AppSettings: DepthOptimizer::Options::init_slants --
    // the initial surface's node slopes from every view's smvs-sgm-slant
    // embedding.  Needs sgm_refine_sweeps > 0 (an error otherwise, before the
    // scene is read); a view whose smvs-sgm map is reused from disk needs its
    // smvs-sgm-slant next to it.  Off by default.
    bool init_slants = false;
    std::size_t num_neighbors = 6, min_neighbors = 3;
    int first_device = 0, num_devices = 1, views_in_flight = 2;
};

struct ReconReport
{
    std::vector<int> reconstructed, skipped_few_neighbors, already_done;
    double seconds = 0.0;
    std::string output_name;
    std::string input_name;      // the embedding the views were read from
    int input_scale = 0;         // as used (the automatic choice resolved)
};

// The body of smvsrecon's main between scene loading and mesh generation
// (app/smvsrecon.cc:400-745): view list, ViewSelection, one ViewQueue task per
// reference view (StereoViews, SGM front end, DepthOptimizer::optimize),
// embeddings saved into the view directories.
ReconReport reconstruct_scene(std::string const& scene_path,
    ReconSettings const& settings);

} // namespace smvs_amd
