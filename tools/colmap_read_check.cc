// Stand-alone check of the COLMAP model reader (csrc/host/colmap_io.cc) under the
// host sanitizers: reads every model directory below the given root -- the
// fixtures of tests/colmap_helpers.py (write_fixtures), the truncated and
// inconsistent ones included -- and exits 0 when every read either succeeded or
// threw; a sanitizer report ends the run with its own status.  Host code only:
// no device, nothing loaded into an interpreter.
//
// Build and run (from the repository root):
//   python -c "import sys; sys.path.insert(0, 'tests'); import colmap_helpers as h; \
//              h.write_fixtures('/tmp/colmap_fixtures')"
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined \
//       -fno-sanitize-recover=undefined -o /tmp/colmap_read_check \
//       tools/colmap_read_check.cc smvs_amd/csrc/host/colmap_io.cc
//   /tmp/colmap_read_check /tmp/colmap_fixtures
#include <dirent.h>
#include <sys/stat.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <exception>
#include <string>
#include <vector>

#include "../smvs_amd/csrc/host/colmap_io.h"

int
main(int argc, char** argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: %s <directory of model directories>\n", argv[0]);
        return 2;
    }
    std::string const root = argv[1];
    DIR* dir = ::opendir(root.c_str());
    if (dir == nullptr) {
        std::fprintf(stderr, "cannot open %s\n", root.c_str());
        return 2;
    }
    std::vector<std::string> names;
    while (struct dirent* e = ::readdir(dir))
        if (e->d_name[0] != '.')
            names.push_back(e->d_name);
    ::closedir(dir);
    std::sort(names.begin(), names.end());
    int read = 0, refused = 0;
    for (std::string const& name : names) {
        std::string const path = root + "/" + name;
        struct stat st;
        if (::stat(path.c_str(), &st) != 0 || !S_ISDIR(st.st_mode))
            continue;
        try {
            smvs_amd::ColmapModel const m = smvs_amd::read_colmap_model(path);
            // walk what was read, and the serialiser, under the sanitizers too
            std::vector<uint8_t> a, b, c;
            smvs_amd::serialize_colmap_model(m, &a, &b, &c);
            for (smvs_amd::ColmapCamera const& cam : m.cameras)
                (void)cam.lens();
            std::printf("read     %-40s %zu cameras, %zu images, %zu points (%s)\n",
                name.c_str(), m.cameras.size(), m.images.size(), m.points.size(),
                m.binary ? "bin" : "txt");
            read += 1;
        } catch (std::exception const& e) {
            std::printf("refused  %-40s %s\n", name.c_str(), e.what());
            refused += 1;
        }
    }
    // the host form of the resampling on a small image, every lens term at work
    {
        smvs_amd::ByteImage::Ptr img = smvs_amd::ByteImage::create(37, 23, 3);
        for (int i = 0; i < 37 * 23 * 3; ++i)
            img->at(i) = (uint8_t)(i * 7);
        smvs_lens const lens = { 30.0f, 29.0f, 18.8f, 11.3f, -0.25f, 0.08f, 0.01f, -0.02f };
        int64_t blank = 0;
        smvs_amd::ByteImage::Ptr out = smvs_amd::undistort_u8(img, lens, 21.0f, 41, 27, &blank);
        std::printf("undistort_u8 37 x 23 x 3 -> %d x %d, %lld blank\n", out->width(),
            out->height(), (long long)blank);
    }
    std::printf("%d read, %d refused\n", read, refused);
    return read >= 2 && refused >= 1 ? 0 : 1;
}
