// maps_check -- the host-only maps unit of the facade (csrc/pf_depth_maps.cpp with pf_image.cpp
// and pf_jpeg.cpp) under a host sanitizer: tests/test_maps_sanitized.py builds this file and those
// units with -fsanitize=address,undefined -fno-sanitize-recover=all and runs it as a child process.
//
//   maps_check <dir> <outdir>
// <dir> holds the image files the test wrote, whole, truncated and empty.  Every file is loaded
// into both map classes, twice into the same object; a map that loaded is read at its corners,
// averaged, saved as 8 bits and moved around.  Per file it prints
//   E <name> <ok> <w> <h> <c> <fnv1a-64 of the float bits>      EquirectangularMap::Load
//   P <name> <ok> <w> <h> <c> <hash>                            PerspectiveMap::Load
//   F<flip><normalize> <name> <ok> <w> <h> <c> <hash>           LoadPfm, for *.pfm
// so the test can hold the sanitized run to the unsanitized library, bit for bit.
#include "../../include/pf_depth.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <filesystem>
#include <utility>

using DepthNamespace::EquirectangularMap;
using DepthNamespace::PerspectiveMap;

template <class Map>
static unsigned long long hash_of(const Map& m)
{
    unsigned long long h = 1469598103934665603ull;
    const size_t n = m.data ? (size_t)m.width * m.height * m.channels * sizeof(float) : 0;
    const unsigned char* b = (const unsigned char*)m.data;
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}

template <class Map>
static void report(const char* tag, const std::string& name, bool ok, const Map& m)
{
    std::printf("%s %s %d %d %d %d %016llx\n", tag, name.c_str(), (int)ok, ok ? m.width : 0,
                ok ? m.height : 0, ok ? m.channels : 0, ok ? hash_of(m) : 0ull);
}

template <class Map>
static float corners(Map& m)
{
    return m.ValueAtXY(0, 0) + m.ValueAtXY(m.width - 1, 0) + m.ValueAtXY(0, m.height - 1) +
           m.ValueAtXY(m.width - 1, m.height - 1);
}

int main(int argc, char* argv[])
{
    if (argc < 3) {
        std::printf("usage: %s <dir> <outdir>\n", argv[0]);
        return 2;
    }
    int failures = 0;
    std::vector<std::string> files;
    for (const auto& e : std::filesystem::directory_iterator(argv[1]))
        files.push_back(e.path().string());
    std::sort(files.begin(), files.end());
    const std::string out(argv[2]);
    for (std::string& fn : files) {
        const std::string name = std::filesystem::path(fn).filename().string();
        {
            EquirectangularMap e;
            const bool first = e.Load(fn), ok = e.Load(fn);
            if (first != ok) ++failures;
            report("E", name, ok, e);
            if (ok) {
                std::string png = out + "/" + name + ".8.png";
                if (!(corners(e) == corners(e)) || !(e.Avg() >= 0) || !e.Save8bit(png)) ++failures;
            }
        }
        if (name.size() > 4 && name.compare(name.size() - 4, 4, ".pfm") == 0)
            for (int flip = 0; flip < 2; ++flip)
                for (int norm = 0; norm < 2; ++norm) {
                    EquirectangularMap e;
                    e.LoadPfm(fn, flip != 0, norm != 0);
                    const bool ok = e.LoadPfm(fn, flip != 0, norm != 0);
                    const char tag[4] = {'F', (char)('0' + flip), (char)('0' + norm), 0};
                    report(tag, name, ok, e);
                    if (ok) (void)corners(e);
                }
        PerspectiveMap p;
        const bool first = p.Load(fn), ok = p.Load(fn);
        if (first != ok) ++failures;
        report("P", name, ok, p);
        if (!ok) continue;
        p.SetWindow(0.1f, 1.2f, 0.8f, 1.9f);
        const unsigned long long h = hash_of(p);
        const float sum = corners(p);
        PerspectiveMap q(std::move(p));  // move-construct: p is left without data
        PerspectiveMap r;
        if (!r.Load(fn)) ++failures;     // r owns an array that the move-assignment must free
        r = std::move(q);
        PerspectiveMap& self = r;
        r = std::move(self);             // onto itself: nothing may be freed
        if (p.data || q.data || !r.window_set || hash_of(r) != h || corners(r) != sum ||
            r.Value(1.0f, 1.0f) != r.ValueAtXY(r.width - 1, r.height - 1))
            ++failures;
    }
    DepthNamespace::Metrics m;
    m.mse_given = 0.25f;
    m.mse_result = 0.16f;
    m.delta1_given = 0.5f;
    m.delta1_result = 0.75f;
    if (!m.Save((out + "/metrics.txt").c_str()) || m.Save((out + "/no/such/dir.txt").c_str()))
        ++failures;
    std::printf(failures ? "maps_check FAILED %d\n" : "maps_check ok\n", failures);
    return failures ? 1 : 0;
}
