// What the translation units of the C ABI (capi_*.cc, entries of host_capi.h)
// share: the error slot and the one guard around every entry, the conversions
// from the C records to the mirror's objects, and the C side of the SGM options.
#pragma once

#include <algorithm>
#include <cstring>
#include <exception>
#include <stdexcept>
#include <string>
#include <vector>

#include "host_capi.h"
#include "sgm_stereo.h"
#include "stereo_view.h"

namespace smvs_amd {
namespace capi {

// the text of smvs_host_last_error: one object per thread for the whole
// library (defined in capi_optimize.cc)
extern thread_local std::string g_host_error;

// Every entry that can fail runs its body in here: a std::exception (and only
// that) becomes the error text and the status -1.
template <class F> int
guarded(F&& body)
{
    try {
        body();
        return 0;
    } catch (std::exception const& e) {
        g_host_error = e.what();
        return -1;
    }
}

// an argument check: std::invalid_argument(text) unless ok
inline void
require(bool ok, std::string const& text)
{
    if (!ok)
        throw std::invalid_argument(text);
}

inline CameraInfo
make_camera(smvs_host_view const& v)
{
    CameraInfo cam;
    cam.flen = v.flen;
    std::copy(v.rot, v.rot + 9, cam.rot);
    std::copy(v.trans, v.trans + 3, cam.trans);
    return cam;
}

inline ByteImage::Ptr
byte_image_from(const uint8_t *pixels, int width, int height, int channels)
{
    ByteImage::Ptr img = ByteImage::create_for_overwrite(width, height, channels);
    std::memcpy(img->begin(), pixels, (std::size_t)width * height * channels);
    return img;
}

// a null pointer for no data
inline FloatImage::Ptr
float_image_from(const float *data, int width, int height, int channels)
{
    if (data == nullptr)
        return nullptr;
    FloatImage::Ptr img = FloatImage::create_for_overwrite(width, height, channels);
    std::memcpy(img->begin(), data, sizeof(float) * (std::size_t)width * height * channels);
    return img;
}

inline StereoView::Ptr
make_view(smvs_host_view const& v, bool linear = false, bool gamma = false)
{
    return StereoView::create(v.view_id, byte_image_from(v.bytes, v.width, v.height,
        v.channels), make_camera(v), linear, gamma);
}

inline std::vector<StereoView::Ptr>
make_views(const smvs_host_view *views, int n)
{
    std::vector<StereoView::Ptr> out;
    for (int j = 0; j < n; ++j)
        out.push_back(make_view(views[j]));
    return out;
}

inline Bundle::Ptr
make_bundle(const smvs_host_bundle *b)
{
    if (b == nullptr)
        return nullptr;
    Bundle::Ptr bundle(new Bundle());
    bundle->features.resize(b->num_features);
    for (int i = 0; i < b->num_features; ++i) {
        std::copy(b->positions + 3 * i, b->positions + 3 * i + 3,
            bundle->features[i].pos);
        bundle->features[i].view_ids.assign(b->ref_views + b->ref_offsets[i],
            b->ref_views + b->ref_offsets[i + 1]);
    }
    return bundle;
}

// The SGM options as the C side states them, in the order the entries take
// them: the loose arguments, then the four optional records (NULL: the
// defaults).  An older entry initialises the members it has arguments for; the
// member initialisers below, which are SGMStereo::Options' own defaults, are the
// only place the rest is written.
struct SgmArgs
{
    int num_steps = SGMStereo::Options().num_steps;
    int subplane = SGMStereo::Options().subplane;
    int num_neighbors = SGMStereo::Options().num_neighbors;
    int consensus = SGMStereo::Options().consensus;
    float agree_ratio = SGMStereo::Options().agree_ratio;
    int min_agree = SGMStereo::Options().min_agree;
    const smvs_host_sgm_sweep *sweep = nullptr;
    const smvs_host_sgm_filter *filter = nullptr;
    const smvs_host_sgm_photo *photo = nullptr;
    const smvs_host_sgm_refine *refine = nullptr;

    bool sweep_on() const { return sweep != nullptr && sweep->sweep != 0; }
};

// The one conversion of the C side into SGMStereo::Options (capi_sgm.cc);
// scale, depth range and device are the caller's.
SGMStereo::Options sgm_options(SgmArgs const& args, bool adaptive_penalty2);

// The range checks of the three records that smvs_host_sgm_depth_* and
// smvs_host_reconstruct_scene_* share, in their order; `family` is the prefix
// of the entry names in the texts ("smvs_host_sgm_depth").
void check_sgm_records(SgmArgs const& args, std::string const& family);

} // namespace capi
} // namespace smvs_amd
