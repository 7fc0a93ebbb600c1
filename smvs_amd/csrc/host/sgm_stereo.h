// Host mirror of smvs::SGMStereo (reference: lib/sgm_stereo.h:21-88).  The
// cost volumes, the 8-path aggregation, the WTA, the left/right check and the
// merge run on the device (smvs_sgm_depth_for_view_raw_opts / _raw_merge, or
// smvs_sgm_sweep_for_view_raw, or with the photo-consistency test the two
// `_raw_photo` entries, with the refinement sweeps the two `_raw_refine`
// entries); the host
// keeps the depth range from the bundle and the image half-sizing.
#pragma once

#include "image.h"
#include "stereo_view.h"

namespace smvs_amd {

class SGMStereo
{
public:
    struct Options  // lib/sgm_stereo.h:24-34
    {
        int debug_lvl = 0;
        int scale = 1;
        // a free integer in the reference; the device takes 2 .. 128 and the
        // multiples of 8 from 136 to 256 (valid_num_steps, include/smvs_hip.h
        // "plane counts") and refuses the rest as an argument error
        int num_steps = 128;
        float min_depth = 0.0f;
        float max_depth = 0.0f;
        uint16_t penalty1 = 6;
        uint16_t penalty2 = 96;
        int device = 0;      // HIP device (not in the reference)
        // not in the reference's Options: selects which of its two builds is
        // reproduced -- false: the SSE build (constant penalty2,
        // lib/sgm_stereo.cc:361-406), true: the build without SSE
        // (penalty2 adapted to the intensity step, lib/sgm_stereo.cc:310-346)
        bool adaptive_penalty2 = false;
        // not in the reference's Options (depth_from_sgm_volume,
        // lib/sgm_stereo.cc:274-306, returns the winning plane's depth): true
        // refines the winner with the parabola through its aggregated cost and
        // its two neighbours' (SMVS_SGM_WINNER_SUBPLANE, include/smvs_hip.h)
        bool subplane = false;
        // not in the reference, whose reconstruct_sgm_depth_for_view looks at
        // the first two neighbours only (app/smvsrecon.cc:360-377):
        // reconstruct_sgm_depth_for_view uses the first min(neighbors.size(),
        // num_neighbors) neighbours.  More than two need `consensus`
        // (SMVS_SGM_MERGE_CONSENSUS, include/smvs_hip.h: per pixel the mean of
        // the largest group of checked depths whose ratio to one of them is at
        // least agree_ratio; no depth with fewer than min_agree of them).
        // 0.95 and 2 are defaults of a user option, not tuned values: at 128
        // planes over a 3 .. 12 range 0.95 admits about two planes at the far
        // end (the left/right check uses 0.8), and nobody has measured their
        // effect on real scenes.
        int num_neighbors = 2;
        bool consensus = false;
        float agree_ratio = 0.95f;
        int min_agree = 2;
        // not in the reference either: the multi-neighbour plane sweep of
        // include/smvs_hip.h (smvs_sgm_sweep_for_view_raw) over the first
        // min(neighbors.size(), num_neighbors) neighbours instead of the runs,
        // the checks and the merge: one cost volume of the main view from all
        // of them (per cell the rounded mean of the sweep_best_k smallest cost
        // bytes, none with fewer than sweep_min_views), one aggregation, one
        // winner, no depth where fewer than sweep_min_support neighbours have
        // a cost of at most sweep_support_cost at the winner plane.  Not
        // together with `consensus`.  -1 stands for the default at n
        // neighbours: min_views = min(2, n), best_k = (n + 1) / 2, min_support =
        // min(2, n).  These and 20 are defaults of a user option, untuned:
        // nobody has measured them on real scenes.
        bool sweep = false;
        int sweep_min_views = -1;
        int sweep_best_k = -1;
        int sweep_support_cost = 20;
        int sweep_min_support = -1;
        // not in the reference either: the two filters of include/smvs_hip.h
        // ("Two single-run rejections") for any of the three front ends above.
        // uniqueness (0 .. 99, a percentage; 0 is off): in the WTA step of every
        // run no depth where a plane more than uniqueness_window (1 .. 256)
        // planes from the winner has a sum r with
        // r * (100 - uniqueness) < S[winner] * 100.  speckle_size (0 and 1 are
        // off): connected components of the final map (4-neighbours whose
        // min / max is at least speckle_ratio) with fewer pixels are removed.
        // (0, 1, 0, 0.95) are defaults of a user option, untuned: nobody has
        // measured them on real scenes.
        int uniqueness = 0;
        int uniqueness_window = 1;
        int speckle_size = 0;
        float speckle_ratio = 0.95f;
        // whether the entries without the filters are called
        bool filters_default() const
        {
            return uniqueness == 0 && uniqueness_window == 1 && speckle_size == 0
                && speckle_ratio == 0.95f;
        }

        // not in the reference either: the multi-view photo-consistency test of
        // include/smvs_hip.h for any of the three front ends above, on the final
        // map of the view and before the speckle removal.  photo_radius (1 .. 3;
        // 0 is off): per pixel and witness the (2 r + 1)^2 window of the main
        // image against its warp into the witness at the pixel's own depth; the
        // confidence is the mean of the photo_best_k largest scores (0: of all),
        // none with fewer than photo_min_views of them, and a depth whose
        // confidence is below photo_min_score is removed (-1 removes nothing).
        // photo_witnesses: how many of the neighbours
        // reconstruct_sgm_depth_for_view is given are witnesses (never fewer
        // than the front end uses); -1: all of them, up to 16.  With the test on
        // the confidence is written as the smvs-sgm-confidence embedding.
        // (0, 2, 2, 0.49, -1) are defaults of a user option, untuned: nobody has
        // measured them on real scenes.
        int photo_radius = 0;
        int photo_best_k = 2;
        int photo_min_views = 2;
        float photo_min_score = 0.49f;
        int photo_witnesses = -1;

        // not in the reference either: the multi-view plane refinement sweeps of
        // include/smvs_hip.h in the photo test's place (they need photo_radius >
        // 0).  refine_sweeps (1 .. 8; 0 is off) red-black sweeps in which a pixel
        // adopts a 4-neighbour's extrapolated plane (depth and two slants) or one
        // of refine_samples (0 .. 8) hashed perturbations of its own -- relative
        // steps refine_depth_step and refine_slant_step, halved per sweep, from
        // refine_seed -- whenever that raises the photo test's confidence;
        // refine_fill = 1 lets a pixel without a depth adopt a neighbour's
        // plane.  With the sweeps on the slants are written as the two-channel
        // smvs-sgm-slant embedding; the optimizer reads them with
        // DepthOptimizer::Options::init_slants only.
        // (0, 2, 0.02, 0.01, 1, 1) are defaults of a user option, untuned: nobody
        // has measured them on real scenes.
        int refine_sweeps = 0;
        int refine_samples = 2;
        float refine_depth_step = 0.02f;
        float refine_slant_step = 0.01f;
        uint32_t refine_seed = 1;
        int refine_fill = 1;
        bool refine_default() const
        {
            return refine_sweeps == 0 && refine_samples == 2 && refine_depth_step == 0.02f
                && refine_slant_step == 0.01f && refine_seed == 1 && refine_fill == 1;
        }

        // the plane counts smvs_sgm_run / smvs_sgm_depth_for_view accept
        static bool valid_num_steps(int n)
        {
            return (n >= 2 && n <= 128) || (n > 128 && n <= 256 && n % 8 == 0);
        }
    };

    SGMStereo(Options const& opts, StereoView::Ptr main,
        StereoView::Ptr neighbor);

    static FloatImage::Ptr reconstruct(Options sgm_opts,
        StereoView::Ptr main_view, StereoView::Ptr neighbor,
        Bundle::ConstPtr bundle = nullptr);

    FloatImage::Ptr run_sgm(float min_depth, float max_depth);

    static void fill_depth_range_for_view(Bundle::ConstPtr bundle,
        StereoView::Ptr view, float* range);

private:
    Options opts;
    StereoView::Ptr main;
    StereoView::Ptr neighbor;
    ByteImage::ConstPtr main_image;
    ByteImage::ConstPtr neighbor_image;
};

// app/smvsrecon.cc:346-384: SGM against the first two neighbours, averaged;
// with Options::consensus against the first Options::num_neighbors, merged by
// consensus; with Options::sweep the plane sweep over them.  More than two
// neighbours with neither, and both together, are std::invalid_argument (never
// a silent truncation).
FloatImage::Ptr reconstruct_sgm_depth_for_view(SGMStereo::Options opts,
    StereoView::Ptr main_view, std::vector<StereoView::Ptr> const& neighbors,
    Bundle::ConstPtr bundle = nullptr);

} // namespace smvs_amd
