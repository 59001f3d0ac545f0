// A caller of include/pf_depth.h for tests/test_gpu_stitch_cli.py: links against
// libpanofuse_depth.so and uses the two diagnostics the facade adds as extensions.
//   stitch_link gpu
//     StitchDepthMaps at 100x50 and 101x51 and CheckLaplacian at 512x256 on the "leres" table's 15
//     windows with hand-filled 64x62 maps (ranges capped as MergeDepthMaps caps them) over a
//     hand-filled 64x32 baseline; prints "STITCH w h <checksum>" per size and "ERR n e0 e1 ..." at
//     %.9g.
#include "../../include/pf_depth.h"

#include <cstdio>
#include <string>
#include <vector>

using DepthNamespace::EquirectangularMap;
using DepthNamespace::PerspectiveMap;

int main(int argc, char** argv)
{
    if (argc < 2 || std::string(argv[1]) != "gpu") return 2;
    std::vector<Vec4f> fovs, ranges;
    if (!pf_named_layout("leres", fovs, ranges)) return 1;
    const int tw = 64, th = 62;
    const double cap = PF_D2R(359.9);
    std::vector<PerspectiveMap> pmaps(fovs.size());
    for (size_t p = 0; p < fovs.size(); ++p) {
        PerspectiveMap& m = pmaps[p];
        m.width = tw;
        m.height = th;
        m.channels = 1;
        m.data = new float[(size_t)tw * th];
        for (int i = 0; i < tw * th; ++i)
            m.data[i] = (float)((i * 37 + (int)p * 11) % 101) / 101.0f;
        m.SetWindow(fovs[p][0], fovs[p][1], fovs[p][2], fovs[p][3]);
        m.ranges[0] = (float)((double)ranges[p][0] < cap ? (double)ranges[p][0] : cap);
        m.ranges[1] = (float)((double)ranges[p][1] < cap ? (double)ranges[p][1] : cap);
        m.ranges[2] = ranges[p][2];
        m.ranges[3] = ranges[p][3];
    }
    const int sizes[2][2] = {{100, 50}, {101, 51}};
    for (auto& s : sizes) {
        int w = s[0], h = s[1];
        std::vector<unsigned short> data((size_t)w * h, 0xFFFF);
        if (!DepthNamespace::StitchDepthMaps(pmaps, data.data(), w, h)) return 1;
        unsigned long long sum = 0;
        for (unsigned short v : data) sum = sum * 1315423911ull + v;
        std::printf("STITCH %d %d %llu\n", w, h, sum);
    }
    EquirectangularMap emap;
    emap.width = 64;
    emap.height = 32;
    emap.channels = 1;
    emap.data = new float[64 * 32];
    for (int i = 0; i < 64 * 32; ++i) emap.data[i] = 0.2f + 0.6f * (float)((i * 37) % 101) / 101.0f;
    std::vector<float> err;
    if (!DepthNamespace::CheckLaplacian(emap, pmaps, 512, 256, g_zenith_range, err)) return 1;
    std::printf("ERR %d", (int)err.size());
    for (float e : err) std::printf(" %.9g", e);
    std::printf("\n");
    return 0;
}
