// A caller of include/pf_depth.h for tests/test_gpu_mask_cli.py: links against
// libpanofuse_depth.so and uses SetTileValidity, the facade's extension for the tile-pixel
// validity rule.
//   valid_link gpu
//     The "leres" table's 15 windows with hand-filled 64x62 maps (ranges capped as MergeDepthMaps
//     caps them) over a hand-filled 64x32 baseline; map 3 holds a block of NaN, map 7 a block of
//     zeros.  Under SetTileValidity(true, 0, inf): StitchDepthMaps at 100x50 and SolveDepthAll at
//     512x256, printed as "STITCH w h <checksum>" / "FUSE w h <checksum>";
//     SolveDepthBySmoothing must refuse ("SMOOTHING refused").  SetTileValidity(true, 1, 0) must
//     fail ("BADRANGE refused").  After SetTileValidity(false, 0, 0) the stitch reads every pixel
//     again: "PLAIN w h <checksum>".
#include "../../include/pf_depth.h"

#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

using DepthNamespace::EquirectangularMap;
using DepthNamespace::PerspectiveMap;

static unsigned long long checksum(const std::vector<unsigned short>& data)
{
    unsigned long long sum = 0;
    for (unsigned short v : data) sum = sum * 1315423911ull + v;
    return sum;
}

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
            m.data[i] = 0.1f + 0.8f * (float)((i * 37 + (int)p * 11) % 101) / 101.0f;
        for (int y = 10; y < 40; ++y)
            for (int x = 20; x < 50; ++x) {
                if (p == 3) m.data[y * tw + x] = NAN;
                if (p == 7) m.data[y * tw + x] = 0.0f;
            }
        m.SetWindow(fovs[p][0], fovs[p][1], fovs[p][2], fovs[p][3]);
        m.ranges[0] = (float)((double)ranges[p][0] < cap ? (double)ranges[p][0] : cap);
        m.ranges[1] = (float)((double)ranges[p][1] < cap ? (double)ranges[p][1] : cap);
        m.ranges[2] = ranges[p][2];
        m.ranges[3] = ranges[p][3];
    }
    EquirectangularMap emap;
    emap.width = 64;
    emap.height = 32;
    emap.channels = 1;
    emap.data = new float[64 * 32];
    for (int i = 0; i < 64 * 32; ++i) emap.data[i] = 0.2f + 0.6f * (float)((i * 37) % 101) / 101.0f;

    if (DepthNamespace::SetTileValidity(true, 1.0f, 0.0f)) return 1;
    std::printf("BADRANGE refused\n");
    if (!DepthNamespace::SetTileValidity(true, 0.0f, INFINITY)) return 1;
    int w = 100, h = 50;
    std::vector<unsigned short> st((size_t)w * h, 0xFFFF);
    if (!DepthNamespace::StitchDepthMaps(pmaps, st.data(), w, h)) return 1;
    std::printf("STITCH %d %d %llu\n", w, h, checksum(st));
    int fw = 512, fh = 256;
    std::vector<unsigned short> fu((size_t)fw * fh, 0xFFFF);
    if (!DepthNamespace::SolveDepthAll(emap, pmaps, fu.data(), fw, fh, g_zenith_range)) return 1;
    std::printf("FUSE %d %d %llu\n", fw, fh, checksum(fu));
    if (DepthNamespace::SolveDepthBySmoothing(pmaps, fu.data(), fw, fh, g_zenith_range)) return 1;
    std::printf("SMOOTHING refused\n");
    if (!DepthNamespace::SetTileValidity(false, 0.0f, 0.0f)) return 1;
    if (!DepthNamespace::StitchDepthMaps(pmaps, st.data(), w, h)) return 1;
    std::printf("PLAIN %d %d %llu\n", w, h, checksum(st));
    return 0;
}
