// C ABI of the host mirror (host_capi.h): COLMAP models as MVE scenes
// (csrc/host/colmap_io.h).
#include "capi_internal.h"

#include "colmap_io.h"

using namespace smvs_amd;
using namespace smvs_amd::capi;

extern "C" int
smvs_host_undistort_u8(const uint8_t *pixels, int width, int height, int channels,
    const smvs_lens *lens, float out_focal, int out_width, int out_height, int device,
    uint8_t *out, int64_t *blank_pixels)
{
    return guarded([&] {
        if (char const* why = undistort_argument_error(pixels, width, height, channels, lens,
                out_focal, out_width, out_height, out))
            throw std::invalid_argument(std::string("smvs_host_undistort_u8: ") + why);
        ByteImage::Ptr img = byte_image_from(pixels, width, height, channels);
        int64_t blank = 0;
        ByteImage::Ptr res = device < 0
            ? undistort_u8(img, *lens, out_focal, out_width, out_height, &blank)
            : undistort_u8_device(img, *lens, out_focal, out_width, out_height, device, &blank);
        std::memcpy(out, res->begin(), (std::size_t)out_width * out_height * channels);
        if (blank_pixels != nullptr)
            *blank_pixels = blank;
    });
}

extern "C" int
smvs_host_read_colmap_model(const char *model_dir, uint8_t *buffer, size_t capacity,
    uint64_t *section_bytes3, int *binary)
{
    // the last model this thread read, serialised: the second call of the
    // size-then-data pair does not read the files again
    static thread_local std::string kept_dir;
    static thread_local std::vector<uint8_t> kept[3];
    static thread_local bool kept_binary = false;
    return guarded([&] {
        require(model_dir != nullptr && section_bytes3 != nullptr,
            "smvs_host_read_colmap_model: bad argument");
        if (buffer == nullptr || kept_dir != model_dir) {
            kept_dir.clear();
            ColmapModel const model = read_colmap_model(model_dir);
            serialize_colmap_model(model, &kept[0], &kept[1], &kept[2]);
            kept_binary = model.binary;
            kept_dir = model_dir;
        }
        std::size_t total = 0;
        for (int i = 0; i < 3; ++i) {
            section_bytes3[i] = kept[i].size();
            total += kept[i].size();
        }
        if (binary != nullptr)
            *binary = kept_binary ? 1 : 0;
        if (buffer != nullptr) {
            require(capacity >= total, "smvs_host_read_colmap_model: buffer too small");
            std::size_t at = 0;
            for (int i = 0; i < 3; ++i) {
                if (!kept[i].empty())
                    std::memcpy(buffer + at, kept[i].data(), kept[i].size());
                at += kept[i].size();
            }
            kept_dir.clear();
            for (int i = 0; i < 3; ++i)
                std::vector<uint8_t>().swap(kept[i]);
        }
    });
}

extern "C" int
smvs_host_import_colmap(const char *model_dir, const char *image_dir, const char *scene_dir,
    const smvs_host_import_settings *o, const int *view_ids, int n_view_ids,
    smvs_host_import_report *report, int max_views, int *view_id, uint32_t *image_id,
    int *whc3, float *flen, int64_t *blank_pixels)
{
    return guarded([&] {
        require(model_dir != nullptr && image_dir != nullptr && scene_dir != nullptr
            && o != nullptr && report != nullptr && (view_ids != nullptr || n_view_ids <= 0)
            && max_views >= 0, "smvs_host_import_colmap: bad argument");
        ImportSettings conf;
        conf.device = o->device;
        conf.zoom = o->zoom;
        conf.out_width = o->out_width;
        conf.out_height = o->out_height;
        conf.container = o->container == 0 ? "png" : o->container == 1 ? "mvei" : "?";
        conf.threads = o->threads;
        conf.overwrite = o->overwrite != 0;
        if (view_ids != nullptr)
            conf.view_ids.assign(view_ids, view_ids + n_view_ids);
        ImportReport const r = import_colmap(model_dir, image_dir, scene_dir, conf);
        report->num_views = r.num_views;
        report->views_written = (int)r.views.size();
        report->points_kept = r.points_kept;
        report->points_dropped = r.points_dropped;
        report->track_elements_kept = r.track_elements_kept;
        report->track_elements_dropped = r.track_elements_dropped;
        report->seconds = r.seconds;
        report->decode_seconds = r.decode_seconds;
        report->undistort_seconds = r.undistort_seconds;
        report->encode_seconds = r.encode_seconds;
        for (std::size_t i = 0; i < r.views.size() && (int)i < max_views; ++i) {
            ImportReport::View const& v = r.views[i];
            if (view_id != nullptr)
                view_id[i] = v.view_id;
            if (image_id != nullptr)
                image_id[i] = v.image_id;
            if (whc3 != nullptr) {
                whc3[3 * i] = v.width;
                whc3[3 * i + 1] = v.height;
                whc3[3 * i + 2] = v.channels;
            }
            if (flen != nullptr)
                flen[i] = v.flen;
            if (blank_pixels != nullptr)
                blank_pixels[i] = v.blank_pixels;
        }
    });
}
