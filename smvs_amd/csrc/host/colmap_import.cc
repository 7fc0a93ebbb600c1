// import_colmap: a COLMAP model and its images as an MVE scene (colmap_io.h)
#include "colmap_io.h"

#include <sys/stat.h>

#include <algorithm>
#include <atomic>
#include <cctype>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <mutex>
#include <stdexcept>
#include <thread>

#include "jpeg_io.h"
#include "png_io.h"
#include "scene_io.h"

namespace smvs_amd {

namespace {

typedef std::chrono::steady_clock Clock;

double
seconds_since(Clock::time_point t0)
{
    return std::chrono::duration<double>(Clock::now() - t0).count();
}

bool
is_directory(std::string const& path)
{
    struct stat st;
    return ::stat(path.c_str(), &st) == 0 && S_ISDIR(st.st_mode);
}

void
make_directory(std::string const& path)
{
    if (is_directory(path))
        return;
    if (::mkdir(path.c_str(), 0777) != 0 && !is_directory(path))
        throw std::runtime_error("cannot create the directory " + path);
}

bool
has_extension(std::string const& path, char const* ext)
{
    std::size_t const n = std::strlen(ext);
    if (path.size() <= n)
        return false;
    for (std::size_t i = 0; i < n; ++i)
        if (std::tolower((unsigned char)path[path.size() - n + i]) != ext[i])
            return false;
    return true;
}

ByteImage::Ptr
decode(std::string const& path)
{
    try {
        if (has_extension(path, ".png"))
            return load_png_u8(path);
        if (has_extension(path, ".jpg") || has_extension(path, ".jpeg"))
            return load_jpeg_u8(path);
    } catch (std::exception const& e) {
        throw std::runtime_error("cannot decode the image " + path + ": " + e.what());
    }
    throw std::runtime_error("cannot decode the image " + path
        + ": neither .png nor .jpg / .jpeg");
}

std::string
format_floats(float const* v, int n)
{
    std::string s;
    char buf[32];
    for (int i = 0; i < n; ++i) {
        std::snprintf(buf, sizeof(buf), i ? " %.9g" : "%.9g", (double)v[i]);
        s += buf;
    }
    return s;
}

// one view of the scene that is written
struct ViewPlan
{
    ColmapImage const* image = nullptr;
    ColmapCamera const* camera = nullptr;
    bool selected = false;
    CameraInfo cam;                  // flen, rot, trans as written
    smvs_lens lens;
    float out_focal = 0.0f;
    int out_width = 0, out_height = 0;
};

// COLMAP's world -> camera pose as MVE's rot / trans: the quaternion normalised
// and turned into R in double, R and t rounded to float once
void
pose_of(ColmapImage const& img, CameraInfo* cam)
{
    double const n = std::sqrt(img.q[0] * img.q[0] + img.q[1] * img.q[1]
        + img.q[2] * img.q[2] + img.q[3] * img.q[3]);
    if (!(n > 0.0) || !std::isfinite(n))
        throw std::runtime_error("image " + std::to_string(img.id) + " (" + img.name
            + ") has no rotation (a zero or non-finite quaternion)");
    double const w = img.q[0] / n, x = img.q[1] / n, y = img.q[2] / n, z = img.q[3] / n;
    double const R[9] = {
        1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
        2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x),
        2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y) };
    for (int i = 0; i < 9; ++i)
        cam->rot[i] = (float)R[i];
    for (int i = 0; i < 3; ++i)
        cam->trans[i] = (float)img.t[i];
}

void
write_meta_ini(std::string const& path, int view_id, std::string const& name,
    CameraInfo const& cam)
{
    std::ofstream out(path.c_str());
    if (!out)
        throw std::runtime_error("cannot write " + path);
    out << "# MVE view meta data is stored in INI-file syntax.\n\n[camera]\n";
    out << "focal_length = " << format_floats(&cam.flen, 1) << "\n";
    out << "pixel_aspect = 1\nprincipal_point = 0.5 0.5\n";
    out << "rotation = " << format_floats(cam.rot, 9) << "\n";
    out << "translation = " << format_floats(cam.trans, 3) << "\n\n";
    out << "[view]\nid = " << view_id << "\nname = " << name << "\n";
    out.close();
    if (!out)
        throw std::runtime_error("write failed: " + path);
}

} // namespace

ByteImage::Ptr
undistort_u8_device(ByteImage::ConstPtr image, smvs_lens const& lens, float out_focal,
    int out_width, int out_height, int device, int64_t* blank_pixels)
{
    if (image == nullptr)
        throw std::invalid_argument("undistort_u8_device: no image");
    int const c = image->channels();
    if (char const* why = undistort_argument_error(image->begin(), image->width(),
            image->height(), c, &lens, out_focal, out_width, out_height, image->begin()))
        throw std::invalid_argument(std::string("undistort_u8_device: ") + why);
    ByteImage::Ptr out = ByteImage::create_for_overwrite(out_width, out_height, c);
    int64_t blank = 0;
    int const rc = smvs_undistort_u8(device, image->begin(), image->width(), image->height(),
        c, &lens, out_focal, out_width, out_height, out->begin(), &blank);
    if (rc == SMVS_ERR_INVALID)
        throw std::invalid_argument(smvs_last_error());
    if (rc != SMVS_OK)
        throw std::runtime_error(smvs_last_error());
    if (blank_pixels != nullptr)
        *blank_pixels = blank;
    return out;
}

ImportReport
import_colmap(std::string const& model_dir, std::string const& image_dir,
    std::string const& scene_dir, ImportSettings const& conf)
{
    Clock::time_point const start = Clock::now();
    if (conf.threads < 1 || conf.threads > 16)
        throw std::invalid_argument("import_colmap: threads must be in [1, 16]");
    if (!(conf.zoom > 0.0f) || !std::isfinite(conf.zoom))
        throw std::invalid_argument("import_colmap: zoom must be positive and finite");
    if (conf.out_width < 0 || conf.out_height < 0
        || (conf.out_width == 0) != (conf.out_height == 0))
        throw std::invalid_argument("import_colmap: out_width and out_height go together");
    if (conf.container != "png" && conf.container != "mvei")
        throw std::invalid_argument("import_colmap: container must be png or mvei");
    if (conf.device < -1)
        throw std::invalid_argument("import_colmap: device must be -1 (host) or a device");
    if (is_directory(scene_dir + "/views") && !conf.overwrite)
        throw std::runtime_error("the scene directory " + scene_dir
            + " already has a views folder (overwrite is not set)");

    ColmapModel const model = read_colmap_model(model_dir);
    if (model.images.empty())
        throw std::runtime_error(model_dir + ": the model has no images");

    // images sorted by IMAGE_ID are the views 0 .. n - 1
    std::vector<ColmapImage const*> order;
    for (ColmapImage const& img : model.images)
        order.push_back(&img);
    std::sort(order.begin(), order.end(),
        [](ColmapImage const* a, ColmapImage const* b) { return a->id < b->id; });
    std::map<uint32_t, ColmapCamera const*> cameras;
    for (ColmapCamera const& c : model.cameras)
        cameras[c.id] = &c;
    std::map<uint32_t, int> view_of_image;
    int const n = (int)order.size();
    std::vector<ViewPlan> plan((std::size_t)n);
    for (int i = 0; i < n; ++i) {
        plan[(std::size_t)i].image = order[(std::size_t)i];
        plan[(std::size_t)i].camera = cameras.at(order[(std::size_t)i]->camera_id);
        plan[(std::size_t)i].selected = conf.view_ids.empty();
    }
    for (int id : conf.view_ids) {
        if (id < 0 || id >= n)
            throw std::invalid_argument("import_colmap: view id " + std::to_string(id)
                + " is not in [0, " + std::to_string(n) + ")");
        plan[(std::size_t)id].selected = true;
    }
    std::vector<int> todo;
    for (int i = 0; i < n; ++i) {
        ViewPlan& v = plan[(std::size_t)i];
        if (!v.selected)
            continue;
        todo.push_back(i);
        view_of_image[v.image->id] = i;
        v.lens = v.camera->lens();
        v.out_width = conf.out_width > 0 ? conf.out_width : (int)v.camera->width;
        v.out_height = conf.out_height > 0 ? conf.out_height : (int)v.camera->height;
        v.out_focal = conf.zoom * v.lens.fx;
        v.cam.flen = v.out_focal / (float)std::max(v.out_width, v.out_height);
        if (!(v.out_focal > 0.0f) || !std::isfinite(v.out_focal))
            throw std::runtime_error("camera " + std::to_string(v.camera->id)
                + " has no positive focal length");
        pose_of(*v.image, &v.cam);
    }

    make_directory(scene_dir);
    make_directory(scene_dir + "/views");

    ImportReport report;
    report.num_views = n;
    report.views.resize(todo.size());
    std::atomic<std::size_t> next(0);
    std::mutex mutex;
    std::exception_ptr error;
    double stage_seconds[3] = { 0.0, 0.0, 0.0 };
    auto worker = [&]() {
        double mine[3] = { 0.0, 0.0, 0.0 };
        for (;;) {
            std::size_t const k = next.fetch_add(1);
            if (k >= todo.size())
                break;
            {
                std::lock_guard<std::mutex> guard(mutex);
                if (error)
                    break;
            }
            try {
                int const view_id = todo[k];
                ViewPlan const& v = plan[(std::size_t)view_id];
                std::string const file = image_dir + "/" + v.image->name;
                Clock::time_point t0 = Clock::now();
                ByteImage::Ptr img = decode(file);
                mine[0] += seconds_since(t0);
                if ((uint64_t)img->width() != v.camera->width
                    || (uint64_t)img->height() != v.camera->height)
                    throw std::runtime_error("the image " + file + " is "
                        + std::to_string(img->width()) + " x " + std::to_string(img->height())
                        + ", its camera " + std::to_string(v.camera->id) + " "
                        + std::to_string(v.camera->width) + " x "
                        + std::to_string(v.camera->height));
                t0 = Clock::now();
                int64_t blank = 0;
                ByteImage::Ptr out = conf.device < 0
                    ? undistort_u8(img, v.lens, v.out_focal, v.out_width, v.out_height, &blank)
                    : undistort_u8_device(img, v.lens, v.out_focal, v.out_width,
                        v.out_height, conf.device, &blank);
                mine[1] += seconds_since(t0);
                t0 = Clock::now();
                char dirname[64];
                std::snprintf(dirname, sizeof(dirname), "/views/view_%04d.mve", view_id);
                std::string const dir = scene_dir + dirname;
                make_directory(dir);
                write_meta_ini(dir + "/meta.ini", view_id, v.image->name, v.cam);
                // (one container per view: a stale copy in the other one would
                // be preferred or shadowed by SceneView::image_path)
                std::remove((dir + "/undistorted.mvei").c_str());
                std::remove((dir + "/undistorted.png").c_str());
                if (conf.container == "png")
                    save_png_u8(dir + "/undistorted.png", out);
                else
                    save_mvei(dir + "/undistorted.mvei", ByteImage::ConstPtr(out));
                mine[2] += seconds_since(t0);
                ImportReport::View& r = report.views[k];
                r.view_id = view_id;
                r.image_id = v.image->id;
                r.name = v.image->name;
                r.width = v.out_width;
                r.height = v.out_height;
                r.channels = out->channels();
                r.flen = v.cam.flen;
                r.blank_pixels = blank;
            } catch (...) {
                std::lock_guard<std::mutex> guard(mutex);
                if (!error)
                    error = std::current_exception();
                break;
            }
        }
        std::lock_guard<std::mutex> guard(mutex);
        for (int s = 0; s < 3; ++s)
            stage_seconds[s] += mine[s];
    };
    {
        std::vector<std::thread> pool;
        int const workers = (int)std::min<std::size_t>((std::size_t)conf.threads, todo.size());
        for (int i = 1; i < workers; ++i)
            pool.emplace_back(worker);
        worker();
        for (std::thread& t : pool)
            t.join();
    }
    if (error)
        std::rethrow_exception(error);
    report.decode_seconds = stage_seconds[0];
    report.undistort_seconds = stage_seconds[1];
    report.encode_seconds = stage_seconds[2];

    // synth_0.out as load_mve_bundle reads it (M28)
    std::string const bundle_path = scene_dir + "/synth_0.out";
    std::vector<ColmapPoint const*> points;
    for (ColmapPoint const& p : model.points)
        points.push_back(&p);
    std::sort(points.begin(), points.end(),
        [](ColmapPoint const* a, ColmapPoint const* b) { return a->id < b->id; });
    std::string features;
    char buf[160];
    for (ColmapPoint const* p : points) {
        std::string refs;
        int kept = 0;
        for (std::size_t k = 0; k < p->image_ids.size(); ++k) {
            auto const it = view_of_image.find(p->image_ids[k]);
            if (it == view_of_image.end()) {
                report.track_elements_dropped += 1;
                continue;
            }
            std::snprintf(buf, sizeof(buf), " %d %u 0", it->second, p->point2d_idx[k]);
            refs += buf;
            kept += 1;
        }
        if (kept == 0) {
            report.points_dropped += 1;
            continue;
        }
        report.points_kept += 1;
        report.track_elements_kept += kept;
        float const pos[3] = { (float)p->xyz[0], (float)p->xyz[1], (float)p->xyz[2] };
        features += format_floats(pos, 3);
        std::snprintf(buf, sizeof(buf), "\n%d %d %d\n%d", (int)p->rgb[0], (int)p->rgb[1],
            (int)p->rgb[2], kept);
        features += buf;
        features += refs;
        features += "\n";
    }
    {
        std::ofstream out(bundle_path.c_str());
        if (!out)
            throw std::runtime_error("cannot write " + bundle_path);
        out << "drews 1.0\n" << n << " " << report.points_kept << "\n";
        for (int i = 0; i < n; ++i) {
            ViewPlan const& v = plan[(std::size_t)i];
            if (!v.selected) {
                // (an invalid camera: a view that was not imported)
                out << "0 0 0\n0 0 0\n0 0 0\n0 0 0\n0 0 0\n";
                continue;
            }
            out << format_floats(&v.cam.flen, 1) << " 0 0\n";
            for (int r = 0; r < 3; ++r)
                out << format_floats(v.cam.rot + 3 * r, 3) << "\n";
            out << format_floats(v.cam.trans, 3) << "\n";
        }
        out << features;
        out.close();
        if (!out)
            throw std::runtime_error("write failed: " + bundle_path);
    }
    report.seconds = seconds_since(start);
    return report;
}

} // namespace smvs_amd
