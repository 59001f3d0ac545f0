// A caller of include/pf_depth.h for tests/test_gpu_planar_cli.py: links against
// libpanofuse_depth.so and uses SetTileDepth, the facade's extension for planar-depth tiles.  A
// plain build, no sanitizer.
//   planar_link gpu
//     The "leres" table's 15 windows with hand-filled 64x62 maps (ranges capped as MergeDepthMaps
//     caps them) over a hand-filled 64x32 baseline.  SetTileDepth(7) must fail ("BADKIND refused").
//     Under SetTileDepth(1): SolveDepthToDepth with map 2 active, printed as "PLANAR a b c d";
//     SolveDisparityToDepth with map 2 active as "PLANARDISP a b c d"; with maps 2 and 3 active
//     SolveDepthToDepth must refuse ("JOINT refused").  After SetTileDepth(0) the same calls are
//     the ray-distance fits again: "RAY a b c d", and the joint solve runs: "JOINT a b c d".
#include "../../include/pf_depth.h"

#include <cstdio>
#include <string>
#include <vector>

using DepthNamespace::EquirectangularMap;
using DepthNamespace::PerspectiveMap;

static void print(const char* tag, const Vec4f& k)
{
    std::printf("%s %.9g %.9g %.9g %.9g\n", tag, k[0], k[1], k[2], k[3]);
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

    std::vector<bool> one(pmaps.size(), false), two(pmaps.size(), false);
    one[2] = true;
    two[2] = two[3] = true;
    Vec4f k;
    if (DepthNamespace::SetTileDepth(7)) return 1;
    std::printf("BADKIND refused\n");
    if (!DepthNamespace::SetTileDepth(1)) return 1;
    if (!DepthNamespace::SolveDepthToDepth(emap, pmaps, one, g_zenith_range, k)) return 1;
    print("PLANAR", k);
    if (!DepthNamespace::SolveDisparityToDepth(emap, pmaps, one, g_zenith_range, k)) return 1;
    print("PLANARDISP", k);
    if (DepthNamespace::SolveDepthToDepth(emap, pmaps, two, g_zenith_range, k)) return 1;
    std::printf("JOINT refused\n");
    if (!DepthNamespace::SetTileDepth(0)) return 1;
    if (!DepthNamespace::SolveDepthToDepth(emap, pmaps, one, g_zenith_range, k)) return 1;
    print("RAY", k);
    if (!DepthNamespace::SolveDepthToDepth(emap, pmaps, two, g_zenith_range, k)) return 1;
    print("JOINT", k);
    return 0;
}
