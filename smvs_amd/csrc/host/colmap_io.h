// COLMAP models as MVE scenes: the reader of a sparse model (cameras, images,
// points3D as .txt or .bin), the host form of the undistortion resampling
// (smvs_undistort_u8, include/smvs_hip.h) and the importer that writes the
// scene directory the rest of this library reads (scene_io.h).  COLMAP is not
// on disk: every format detail is recalled, [COLMAP-unverified], rows C1..C9 of
// tests/golden/COLMAP.md.  Nothing here has a counterpart in the reference.
//
// colmap_io.cc (reader, host undistortion) depends on nothing else of the
// library, so that it can be built on its own under a sanitizer
// (tools/colmap_read_check.cc); colmap_import.cc holds the importer.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "image.h"
#include "../../../include/smvs_hip.h"

namespace smvs_amd {

// COLMAP's camera model ids (C2).  The first five are read: one lens form
// (smvs_lens) covers them; the others are an error that names them.
enum ColmapCameraModel
{
    COLMAP_SIMPLE_PINHOLE = 0, COLMAP_PINHOLE = 1, COLMAP_SIMPLE_RADIAL = 2,
    COLMAP_RADIAL = 3, COLMAP_OPENCV = 4, COLMAP_OPENCV_FISHEYE = 5,
    COLMAP_FULL_OPENCV = 6, COLMAP_FOV = 7, COLMAP_SIMPLE_RADIAL_FISHEYE = 8,
    COLMAP_RADIAL_FISHEYE = 9, COLMAP_THIN_PRISM_FISHEYE = 10
};
// number of parameters of a model that is read, -1 for the others
int colmap_model_num_params(int model);

struct ColmapCamera
{
    uint32_t id = 0;
    int model = 0;
    uint64_t width = 0, height = 0;
    std::vector<double> params;
    // the model's parameters as the one lens form, rounded to float once
    smvs_lens lens(void) const;
};

struct ColmapImage
{
    uint32_t id = 0;
    double q[4] = { 1, 0, 0, 0 };   // w, x, y, z: world -> camera
    double t[3] = { 0, 0, 0 };
    uint32_t camera_id = 0;
    std::string name;
    std::vector<double> xy;             // 2 per 2D point
    std::vector<int64_t> point3d_ids;   // -1: no 3D point
};

struct ColmapPoint
{
    uint64_t id = 0;
    double xyz[3] = { 0, 0, 0 };
    uint8_t rgb[3] = { 0, 0, 0 };
    double error = 0.0;
    std::vector<uint32_t> image_ids, point2d_idx;   // the track
};

struct ColmapModel
{
    std::vector<ColmapCamera> cameras;   // in the file's order
    std::vector<ColmapImage> images;
    std::vector<ColmapPoint> points;
    bool binary = false;                 // read from the .bin files
};

// cameras / images / points3D of `dir`: the .bin files if all three exist, else
// the .txt files.  Throws std::runtime_error naming the file for a file that is
// missing, truncated or inconsistent (a count that overruns the file, an
// unterminated name, a duplicate id, an image whose camera does not exist) and
// for a camera model that is not read (naming the model and the camera).  No
// size read from a file is used for an allocation before it is checked against
// the file's length.
ColmapModel read_colmap_model(std::string const& dir);
// the three sections in the binary layout (C6-C8), for the C interface
void serialize_colmap_model(ColmapModel const& model, std::vector<uint8_t>* cameras,
    std::vector<uint8_t>* images, std::vector<uint8_t>* points);

// The host form of smvs_undistort_u8 (csrc/host/undistort_math.h, shared with
// the kernel): the same bytes and the same blank count.  Throws
// std::invalid_argument for what the device entry refuses.
ByteImage::Ptr undistort_u8(ByteImage::ConstPtr image, smvs_lens const& lens,
    float out_focal, int out_width, int out_height, int64_t* blank_pixels = nullptr);
// what smvs_undistort_u8 refuses (the reason), or nullptr
char const* undistort_argument_error(const uint8_t* pixels, int width, int height,
    int channels, const smvs_lens* lens, float out_focal, int out_width, int out_height,
    const uint8_t* out);
// ... on device `device` (smvs_undistort_u8); std::runtime_error for a device error
ByteImage::Ptr undistort_u8_device(ByteImage::ConstPtr image, smvs_lens const& lens,
    float out_focal, int out_width, int out_height, int device,
    int64_t* blank_pixels = nullptr);

struct ImportSettings
{
    int device = -1;                 // -1: the host form
    float zoom = 1.0f;               // out_focal = zoom * fx
    int out_width = 0, out_height = 0;   // 0: the input's
    std::string container = "png";   // "png" or "mvei": the `undistorted` embedding
    int threads = 4;                 // host workers decode -> undistort -> encode, 1..16
    std::vector<int> view_ids;       // empty: every image; else these views only
    bool overwrite = false;          // write into a scene that has a views folder
};

struct ImportReport
{
    struct View
    {
        int view_id = 0;
        uint32_t image_id = 0;
        std::string name;
        int width = 0, height = 0, channels = 0;
        float flen = 0.0f;
        int64_t blank_pixels = 0;
    };
    std::vector<View> views;         // the views written, by view id
    int num_views = 0;               // images of the model (= cameras in synth_0.out)
    int64_t points_kept = 0, points_dropped = 0;
    int64_t track_elements_kept = 0, track_elements_dropped = 0;
    // wall time, and the workers' time by stage, summed over the workers
    double seconds = 0.0, decode_seconds = 0.0, undistort_seconds = 0.0,
        encode_seconds = 0.0;
};

// The model of `model_dir` with the images of `image_dir` as the MVE scene
// `scene_dir`: the images sorted by IMAGE_ID are the views 0 .. n - 1, each
// resampled into a pinhole camera with a centred principal point and written as
// views/view_%04d.mve/{meta.ini, undistorted.<container>}; the poses are
// COLMAP's world -> camera (MVE's rot / trans, M11); synth_0.out holds the
// cameras in view order and the 3D points sorted by id with their tracks as
// (view id, POINT2D_IDX, 0).  Throws std::invalid_argument for bad settings,
// std::runtime_error naming the file for what cannot be read or decoded and for
// an image whose size differs from its camera's.
ImportReport import_colmap(std::string const& model_dir, std::string const& image_dir,
    std::string const& scene_dir, ImportSettings const& settings);

} // namespace smvs_amd
