#include "colmap_io.h"

#include <sys/stat.h>

#include <algorithm>
#include <cctype>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <set>
#include <stdexcept>

#include "undistort_math.h"

namespace smvs_amd {

namespace {

struct ModelInfo { int id; char const* name; int num_params; bool read; };
// COLMAP's src/base/camera_models.h [COLMAP-unverified C2]
ModelInfo const MODELS[] = {
    { COLMAP_SIMPLE_PINHOLE, "SIMPLE_PINHOLE", 3, true },
    { COLMAP_PINHOLE, "PINHOLE", 4, true },
    { COLMAP_SIMPLE_RADIAL, "SIMPLE_RADIAL", 4, true },
    { COLMAP_RADIAL, "RADIAL", 5, true },
    { COLMAP_OPENCV, "OPENCV", 8, true },
    { COLMAP_OPENCV_FISHEYE, "OPENCV_FISHEYE", 8, false },
    { COLMAP_FULL_OPENCV, "FULL_OPENCV", 12, false },
    { COLMAP_FOV, "FOV", 5, false },
    { COLMAP_SIMPLE_RADIAL_FISHEYE, "SIMPLE_RADIAL_FISHEYE", 4, false },
    { COLMAP_RADIAL_FISHEYE, "RADIAL_FISHEYE", 5, false },
    { COLMAP_THIN_PRISM_FISHEYE, "THIN_PRISM_FISHEYE", 12, false },
};

ModelInfo const*
model_info(int model)
{
    for (ModelInfo const& m : MODELS)
        if (m.id == model)
            return &m;
    return nullptr;
}

uint64_t const MAX_IMAGE_SIDE = (uint64_t)1 << 20;

[[noreturn]] void
fail(std::string const& file, std::string const& what)
{
    throw std::runtime_error(file + ": " + what);
}

bool
file_exists(std::string const& path)
{
    struct stat st;
    return ::stat(path.c_str(), &st) == 0 && S_ISREG(st.st_mode);
}

// the checks both formats share, once a camera's fields are known
void
check_camera(std::string const& file, ColmapCamera const& cam)
{
    ModelInfo const* info = model_info(cam.model);
    if (info == nullptr)
        fail(file, "camera " + std::to_string(cam.id) + " has the unknown camera model id "
            + std::to_string(cam.model));
    if (!info->read)
        fail(file, "camera " + std::to_string(cam.id) + " has the camera model "
            + info->name + ", which is not supported (SIMPLE_PINHOLE, PINHOLE, SIMPLE_RADIAL, "
            "RADIAL and OPENCV are)");
    if (cam.width < 1 || cam.height < 1 || cam.width > MAX_IMAGE_SIDE
        || cam.height > MAX_IMAGE_SIDE)
        fail(file, "camera " + std::to_string(cam.id) + " has an impossible image size");
    if ((int)cam.params.size() != info->num_params)
        fail(file, "camera " + std::to_string(cam.id) + " (" + info->name + ") has "
            + std::to_string(cam.params.size()) + " parameters, not "
            + std::to_string(info->num_params));
}

// ------------------------------------------------------------------ text

std::vector<std::string>
split(std::string const& line)
{
    std::vector<std::string> tokens;
    std::size_t i = 0;
    while (i < line.size()) {
        while (i < line.size() && std::isspace((unsigned char)line[i]))
            ++i;
        std::size_t const a = i;
        while (i < line.size() && !std::isspace((unsigned char)line[i]))
            ++i;
        if (i > a)
            tokens.push_back(line.substr(a, i - a));
    }
    return tokens;
}

double
to_double(std::string const& file, std::string const& token)
{
    char* end = nullptr;
    errno = 0;
    double const v = std::strtod(token.c_str(), &end);
    if (token.empty() || end != token.c_str() + token.size())
        fail(file, "'" + token + "' is not a number");
    return v;
}

int64_t
to_int(std::string const& file, std::string const& token, int64_t lo, int64_t hi)
{
    char* end = nullptr;
    errno = 0;
    long long const v = std::strtoll(token.c_str(), &end, 10);
    if (token.empty() || end != token.c_str() + token.size() || errno == ERANGE)
        fail(file, "'" + token + "' is not an integer");
    if (v < lo || v > hi)
        fail(file, "'" + token + "' is out of range");
    return (int64_t)v;
}

bool
is_blank_or_comment(std::string const& line)
{
    std::size_t const a = line.find_first_not_of(" \t\r\n");
    return a == std::string::npos || line[a] == '#';
}

void
strip_cr(std::string* line)
{
    while (!line->empty() && (line->back() == '\r' || line->back() == '\n'))
        line->pop_back();
}

std::ifstream
open_text(std::string const& path)
{
    std::ifstream in(path.c_str());
    if (!in)
        fail(path, "cannot open");
    return in;
}

void
read_cameras_text(std::string const& path, ColmapModel* model)
{
    std::ifstream in = open_text(path);
    std::string line;
    while (std::getline(in, line)) {
        if (is_blank_or_comment(line))
            continue;
        std::vector<std::string> const tok = split(line);
        if (tok.size() < 4)
            fail(path, "a camera line with fewer than four fields");
        ColmapCamera cam;
        cam.id = (uint32_t)to_int(path, tok[0], 0, UINT32_MAX);
        cam.model = -1;
        for (ModelInfo const& m : MODELS)
            if (tok[1] == m.name)
                cam.model = m.id;
        if (cam.model < 0)
            fail(path, "camera " + tok[0] + " has the unknown camera model " + tok[1]);
        cam.width = (uint64_t)to_int(path, tok[2], 0, INT64_MAX);
        cam.height = (uint64_t)to_int(path, tok[3], 0, INT64_MAX);
        for (std::size_t i = 4; i < tok.size(); ++i)
            cam.params.push_back(to_double(path, tok[i]));
        check_camera(path, cam);
        model->cameras.push_back(cam);
    }
}

void
read_images_text(std::string const& path, ColmapModel* model)
{
    std::ifstream in = open_text(path);
    std::string line;
    while (std::getline(in, line)) {
        if (is_blank_or_comment(line))
            continue;
        strip_cr(&line);
        // IMAGE_ID QW QX QY QZ TX TY TZ CAMERA_ID NAME, NAME the rest of the line
        ColmapImage img;
        std::size_t pos = 0;
        std::string field[9];
        for (int i = 0; i < 9; ++i) {
            while (pos < line.size() && std::isspace((unsigned char)line[pos]))
                ++pos;
            std::size_t const a = pos;
            while (pos < line.size() && !std::isspace((unsigned char)line[pos]))
                ++pos;
            if (pos == a)
                fail(path, "an image line with fewer than ten fields");
            field[i] = line.substr(a, pos - a);
        }
        while (pos < line.size() && std::isspace((unsigned char)line[pos]))
            ++pos;
        img.name = line.substr(pos);
        if (img.name.empty())
            fail(path, "image " + field[0] + " has no name");
        img.id = (uint32_t)to_int(path, field[0], 0, UINT32_MAX);
        for (int i = 0; i < 4; ++i)
            img.q[i] = to_double(path, field[1 + i]);
        for (int i = 0; i < 3; ++i)
            img.t[i] = to_double(path, field[5 + i]);
        img.camera_id = (uint32_t)to_int(path, field[8], 0, UINT32_MAX);
        // the points line: X Y POINT3D_ID triples; it may be empty, but it is there
        if (!std::getline(in, line))
            fail(path, "image " + field[0] + " has no line of 2D points (truncated)");
        std::vector<std::string> const tok = split(line);
        if (tok.size() % 3 != 0)
            fail(path, "the 2D points of image " + field[0] + " are not X Y POINT3D_ID triples");
        for (std::size_t i = 0; i < tok.size(); i += 3) {
            img.xy.push_back(to_double(path, tok[i]));
            img.xy.push_back(to_double(path, tok[i + 1]));
            img.point3d_ids.push_back(to_int(path, tok[i + 2], -1, INT64_MAX));
        }
        model->images.push_back(img);
    }
}

void
read_points_text(std::string const& path, ColmapModel* model)
{
    std::ifstream in = open_text(path);
    std::string line;
    while (std::getline(in, line)) {
        if (is_blank_or_comment(line))
            continue;
        std::vector<std::string> const tok = split(line);
        if (tok.size() < 8 || (tok.size() - 8) % 2 != 0)
            fail(path, "a point line that is not POINT3D_ID X Y Z R G B ERROR "
                "(IMAGE_ID POINT2D_IDX)*");
        ColmapPoint p;
        p.id = (uint64_t)to_int(path, tok[0], 0, INT64_MAX);
        for (int i = 0; i < 3; ++i)
            p.xyz[i] = to_double(path, tok[1 + i]);
        for (int i = 0; i < 3; ++i)
            p.rgb[i] = (uint8_t)to_int(path, tok[4 + i], 0, 255);
        p.error = to_double(path, tok[7]);
        for (std::size_t i = 8; i < tok.size(); i += 2) {
            p.image_ids.push_back((uint32_t)to_int(path, tok[i], 0, UINT32_MAX));
            p.point2d_idx.push_back((uint32_t)to_int(path, tok[i + 1], 0, UINT32_MAX));
        }
        model->points.push_back(p);
    }
}

// ---------------------------------------------------------------- binary

// A whole file in memory and a cursor that never leaves it
struct Bytes
{
    std::string file;
    std::vector<uint8_t> data;
    std::size_t pos = 0;

    explicit Bytes(std::string const& path) : file(path)
    {
        std::ifstream in(path.c_str(), std::ios::binary);
        if (!in)
            fail(path, "cannot open");
        in.seekg(0, std::ios::end);
        std::streamoff const n = in.tellg();
        if (n < 0)
            fail(path, "cannot read");
        in.seekg(0, std::ios::beg);
        data.resize((std::size_t)n);
        if (n > 0)
            in.read(reinterpret_cast<char*>(data.data()), n);
        if (!in)
            fail(path, "cannot read");
    }
    std::size_t left(void) const { return data.size() - pos; }
    void need(std::size_t n, char const* what) const
    {
        if (n > left())
            fail(file, std::string("truncated in ") + what);
    }
    template <typename T> T get(char const* what)
    {
        need(sizeof(T), what);
        T v;
        std::memcpy(&v, data.data() + pos, sizeof(T));   // (little endian, as the host)
        pos += sizeof(T);
        return v;
    }
    // `count` records of at least `min_bytes` each have to fit into what is left
    void check_count(uint64_t count, std::size_t min_bytes, char const* what) const
    {
        if (count > left() / min_bytes)
            fail(file, std::string("the number of ") + what + " ("
                + std::to_string(count) + ") overruns the file");
    }
    void done(void) const
    {
        if (left() != 0)
            fail(file, std::to_string(left()) + " bytes behind the last record");
    }
};

void
read_cameras_binary(std::string const& path, ColmapModel* model)
{
    Bytes in(path);
    uint64_t const n = in.get<uint64_t>("the camera count");
    in.check_count(n, 4 + 4 + 8 + 8, "cameras");
    model->cameras.reserve((std::size_t)n);
    for (uint64_t i = 0; i < n; ++i) {
        ColmapCamera cam;
        cam.id = in.get<uint32_t>("a camera");
        cam.model = in.get<int32_t>("a camera");
        cam.width = in.get<uint64_t>("a camera");
        cam.height = in.get<uint64_t>("a camera");
        ModelInfo const* info = model_info(cam.model);
        // (an unknown or unsupported model: check_camera names it)
        if (info != nullptr && info->read)
            for (int k = 0; k < info->num_params; ++k)
                cam.params.push_back(in.get<double>("a camera's parameters"));
        check_camera(path, cam);
        model->cameras.push_back(cam);
    }
    in.done();
}

void
read_images_binary(std::string const& path, ColmapModel* model)
{
    Bytes in(path);
    uint64_t const n = in.get<uint64_t>("the image count");
    // id, q, t, camera id, an empty name's terminator, the 2D point count
    in.check_count(n, 4 + 32 + 24 + 4 + 1 + 8, "images");
    model->images.reserve((std::size_t)n);
    for (uint64_t i = 0; i < n; ++i) {
        ColmapImage img;
        img.id = in.get<uint32_t>("an image");
        for (int k = 0; k < 4; ++k)
            img.q[k] = in.get<double>("an image");
        for (int k = 0; k < 3; ++k)
            img.t[k] = in.get<double>("an image");
        img.camera_id = in.get<uint32_t>("an image");
        void const* zero = std::memchr(in.data.data() + in.pos, 0, in.left());
        if (zero == nullptr)
            fail(path, "the name of image " + std::to_string(img.id) + " is not terminated");
        std::size_t const len = (std::size_t)(static_cast<uint8_t const*>(zero)
            - (in.data.data() + in.pos));
        img.name.assign(reinterpret_cast<char const*>(in.data.data() + in.pos), len);
        in.pos += len + 1;
        if (img.name.empty())
            fail(path, "image " + std::to_string(img.id) + " has no name");
        uint64_t const m = in.get<uint64_t>("an image's 2D point count");
        in.check_count(m, 24, "2D points of an image");
        img.xy.reserve((std::size_t)m * 2);
        img.point3d_ids.reserve((std::size_t)m);
        for (uint64_t k = 0; k < m; ++k) {
            img.xy.push_back(in.get<double>("a 2D point"));
            img.xy.push_back(in.get<double>("a 2D point"));
            uint64_t const pid = in.get<uint64_t>("a 2D point");
            if (pid != UINT64_MAX && pid > (uint64_t)INT64_MAX)
                fail(path, "a POINT3D_ID of image " + std::to_string(img.id)
                    + " is out of range");
            img.point3d_ids.push_back(pid == UINT64_MAX ? (int64_t)-1 : (int64_t)pid);
        }
        model->images.push_back(std::move(img));
    }
    in.done();
}

void
read_points_binary(std::string const& path, ColmapModel* model)
{
    Bytes in(path);
    uint64_t const n = in.get<uint64_t>("the point count");
    in.check_count(n, 8 + 24 + 3 + 8 + 8, "points");
    model->points.reserve((std::size_t)n);
    for (uint64_t i = 0; i < n; ++i) {
        ColmapPoint p;
        p.id = in.get<uint64_t>("a point");
        for (int k = 0; k < 3; ++k)
            p.xyz[k] = in.get<double>("a point");
        for (int k = 0; k < 3; ++k)
            p.rgb[k] = in.get<uint8_t>("a point");
        p.error = in.get<double>("a point");
        uint64_t const len = in.get<uint64_t>("a point's track length");
        in.check_count(len, 8, "track elements of a point");
        p.image_ids.reserve((std::size_t)len);
        p.point2d_idx.reserve((std::size_t)len);
        for (uint64_t k = 0; k < len; ++k) {
            p.image_ids.push_back(in.get<uint32_t>("a track"));
            p.point2d_idx.push_back(in.get<uint32_t>("a track"));
        }
        model->points.push_back(std::move(p));
    }
    in.done();
}

template <typename T>
void
put(std::vector<uint8_t>* out, T v)
{
    uint8_t raw[sizeof(T)];
    std::memcpy(raw, &v, sizeof(T));
    out->insert(out->end(), raw, raw + sizeof(T));
}

} // namespace

int
colmap_model_num_params(int model)
{
    ModelInfo const* info = model_info(model);
    return info && info->read ? info->num_params : -1;
}

smvs_lens
ColmapCamera::lens(void) const
{
    if ((int)params.size() != colmap_model_num_params(model))
        throw std::invalid_argument("ColmapCamera::lens: not a camera that is read");
    std::vector<double> const& p = params;
    smvs_lens l = { 0, 0, 0, 0, 0, 0, 0, 0 };
    switch (model) {
    case COLMAP_SIMPLE_PINHOLE:
        l.fx = l.fy = (float)p[0]; l.cx = (float)p[1]; l.cy = (float)p[2];
        break;
    case COLMAP_PINHOLE:
        l.fx = (float)p[0]; l.fy = (float)p[1]; l.cx = (float)p[2]; l.cy = (float)p[3];
        break;
    case COLMAP_SIMPLE_RADIAL:
        l.fx = l.fy = (float)p[0]; l.cx = (float)p[1]; l.cy = (float)p[2];
        l.k1 = (float)p[3];
        break;
    case COLMAP_RADIAL:
        l.fx = l.fy = (float)p[0]; l.cx = (float)p[1]; l.cy = (float)p[2];
        l.k1 = (float)p[3]; l.k2 = (float)p[4];
        break;
    default:   // COLMAP_OPENCV
        l.fx = (float)p[0]; l.fy = (float)p[1]; l.cx = (float)p[2]; l.cy = (float)p[3];
        l.k1 = (float)p[4]; l.k2 = (float)p[5]; l.p1 = (float)p[6]; l.p2 = (float)p[7];
        break;
    }
    return l;
}

ColmapModel
read_colmap_model(std::string const& dir)
{
    ColmapModel model;
    model.binary = file_exists(dir + "/cameras.bin") && file_exists(dir + "/images.bin")
        && file_exists(dir + "/points3D.bin");
    if (model.binary) {
        read_cameras_binary(dir + "/cameras.bin", &model);
        read_images_binary(dir + "/images.bin", &model);
        read_points_binary(dir + "/points3D.bin", &model);
    } else {
        read_cameras_text(dir + "/cameras.txt", &model);
        read_images_text(dir + "/images.txt", &model);
        read_points_text(dir + "/points3D.txt", &model);
    }
    // across the files
    std::string const ext = model.binary ? ".bin" : ".txt";
    std::set<uint32_t> camera_ids;
    for (ColmapCamera const& c : model.cameras)
        if (!camera_ids.insert(c.id).second)
            fail(dir + "/cameras" + ext, "camera id " + std::to_string(c.id) + " appears twice");
    std::set<uint32_t> image_ids;
    for (ColmapImage const& i : model.images) {
        if (!image_ids.insert(i.id).second)
            fail(dir + "/images" + ext, "image id " + std::to_string(i.id) + " appears twice");
        if (camera_ids.count(i.camera_id) == 0)
            fail(dir + "/images" + ext, "image " + std::to_string(i.id) + " (" + i.name
                + ") has the camera id " + std::to_string(i.camera_id)
                + ", which cameras" + ext + " does not hold");
    }
    std::set<uint64_t> point_ids;
    for (ColmapPoint const& p : model.points)
        if (!point_ids.insert(p.id).second)
            fail(dir + "/points3D" + ext, "point id " + std::to_string(p.id) + " appears twice");
    return model;
}

void
serialize_colmap_model(ColmapModel const& model, std::vector<uint8_t>* cameras,
    std::vector<uint8_t>* images, std::vector<uint8_t>* points)
{
    cameras->clear();
    images->clear();
    points->clear();
    put<uint64_t>(cameras, model.cameras.size());
    for (ColmapCamera const& c : model.cameras) {
        put<uint32_t>(cameras, c.id);
        put<int32_t>(cameras, c.model);
        put<uint64_t>(cameras, c.width);
        put<uint64_t>(cameras, c.height);
        for (double v : c.params)
            put<double>(cameras, v);
    }
    put<uint64_t>(images, model.images.size());
    for (ColmapImage const& i : model.images) {
        put<uint32_t>(images, i.id);
        for (double v : i.q)
            put<double>(images, v);
        for (double v : i.t)
            put<double>(images, v);
        put<uint32_t>(images, i.camera_id);
        images->insert(images->end(), i.name.begin(), i.name.end());
        images->push_back(0);
        put<uint64_t>(images, i.point3d_ids.size());
        for (std::size_t k = 0; k < i.point3d_ids.size(); ++k) {
            put<double>(images, i.xy[2 * k]);
            put<double>(images, i.xy[2 * k + 1]);
            put<uint64_t>(images, i.point3d_ids[k] < 0 ? UINT64_MAX
                                                       : (uint64_t)i.point3d_ids[k]);
        }
    }
    put<uint64_t>(points, model.points.size());
    for (ColmapPoint const& p : model.points) {
        put<uint64_t>(points, p.id);
        for (double v : p.xyz)
            put<double>(points, v);
        for (uint8_t v : p.rgb)
            put<uint8_t>(points, v);
        put<double>(points, p.error);
        put<uint64_t>(points, p.image_ids.size());
        for (std::size_t k = 0; k < p.image_ids.size(); ++k) {
            put<uint32_t>(points, p.image_ids[k]);
            put<uint32_t>(points, p.point2d_idx[k]);
        }
    }
}

char const*
undistort_argument_error(const uint8_t* pixels, int width, int height, int channels,
    const smvs_lens* lens, float out_focal, int out_width, int out_height,
    const uint8_t* out)
{
    if (pixels == nullptr || lens == nullptr || out == nullptr)
        return "null argument";
    if (channels < 1 || channels > 4)
        return "1 to 4 channels";
    if (width < 1 || height < 1 || out_width < 1 || out_height < 1)
        return "a size below 1";
    if (!(out_focal > 0.0f) || !std::isfinite(out_focal))
        return "out_focal must be positive and finite";
    float const v[8] = { lens->fx, lens->fy, lens->cx, lens->cy, lens->k1, lens->k2,
        lens->p1, lens->p2 };
    for (float f : v)
        if (!std::isfinite(f))
            return "non-finite lens value";
    std::size_t const limit = (std::size_t)1 << 31;
    if (width > (1 << 20) || height > (1 << 20) || out_width > (1 << 20)
        || out_height > (1 << 20)
        || (std::size_t)width * (std::size_t)height * (std::size_t)channels > limit
        || (std::size_t)out_width * (std::size_t)out_height * (std::size_t)channels > limit)
        return "image too large";
    return nullptr;
}

ByteImage::Ptr
undistort_u8(ByteImage::ConstPtr image, smvs_lens const& lens, float out_focal,
    int out_width, int out_height, int64_t* blank_pixels)
{
    if (image == nullptr)
        throw std::invalid_argument("undistort_u8: no image");
    int const w = image->width(), h = image->height(), c = image->channels();
    uint8_t const* src = image->begin();
    // (`src` stands in for the output pointer: it is allocated below)
    if (char const* why = undistort_argument_error(src, w, h, c, &lens, out_focal,
            out_width, out_height, src))
        throw std::invalid_argument(std::string("undistort_u8: ") + why);
    smvs_undistort::Mapping const m = smvs_undistort::make_mapping(lens.fx, lens.fy, lens.cx,
        lens.cy, lens.k1, lens.k2, lens.p1, lens.p2, w, h, out_focal, out_width, out_height);
    ByteImage::Ptr out = ByteImage::create_for_overwrite(out_width, out_height, c);
    uint8_t* dst = out->begin();
    int64_t blank = 0;
    for (int y = 0; y < out_height; ++y)
        for (int x = 0; x < out_width; ++x) {
            float sx, sy;
            if (smvs_undistort::source_position(m, x, y, &sx, &sy)) {
                smvs_undistort::Taps const t = smvs_undistort::make_taps(m, c, sx, sy);
                for (int ch = 0; ch < c; ++ch)
                    *dst++ = smvs_undistort::sample(src, t, ch);
            } else {
                for (int ch = 0; ch < c; ++ch)
                    *dst++ = 0;
                blank += 1;
            }
        }
    if (blank_pixels != nullptr)
        *blank_pixels = blank;
    return out;
}

} // namespace smvs_amd
