// A caller of include/pf_depth.h for tests/test_gpu_consist_cli.py: links against
// libpanofuse_depth.so and uses the facade's two extensions of the overlap-consistent registration.
// A plain build, no sanitizer.
//   consist_link gpu
//     The "leres" table's 15 windows with hand-filled 64x62 maps (ranges capped as MergeDepthMaps
//     caps them) over a hand-filled 64x32 baseline.  SolveDepthToDepthConsistent with lambda -1
//     must fail ("BADLAMBDA refused"), and under SetTileDepth(1) too ("PLANAR refused").  Then with
//     lambda 1: "CONS <map> a b c d" per map; TileOverlapStats of the maps as they are as
//     "RAW <p> <q> count sum sum_sq max_abs nan_count" per pair, under the coefficients as "FIT ...".
#include "../../include/pf_depth.h"

#include <cstdio>
#include <string>
#include <vector>

using DepthNamespace::EquirectangularMap;
using DepthNamespace::PerspectiveMap;
using DepthNamespace::TileOverlapStat;

static void print(const char* tag, const std::vector<TileOverlapStat>& st)
{
    for (const TileOverlapStat& s : st)
        std::printf("%s %d %d %.17g %.17g %.17g %.17g %.17g\n", tag, s.p, s.q, s.count, s.sum,
                    s.sum_sq, s.max_abs, s.nan_count);
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

    std::vector<Vec4f> abcd, none;
    if (DepthNamespace::SolveDepthToDepthConsistent(emap, pmaps, g_zenith_range, -1.0, abcd)) return 1;
    std::printf("BADLAMBDA refused\n");
    if (!DepthNamespace::SetTileDepth(1)) return 1;
    if (DepthNamespace::SolveDepthToDepthConsistent(emap, pmaps, g_zenith_range, 1.0, abcd)) return 1;
    std::printf("PLANAR refused\n");
    if (!DepthNamespace::SetTileDepth(0)) return 1;
    if (!DepthNamespace::SolveDepthToDepthConsistent(emap, pmaps, g_zenith_range, 1.0, abcd)) return 1;
    if (abcd.size() != pmaps.size()) return 1;
    for (size_t p = 0; p < abcd.size(); ++p)
        std::printf("CONS %zu %.9g %.9g %.9g %.9g\n", p, abcd[p][0], abcd[p][1], abcd[p][2],
                    abcd[p][3]);
    std::vector<TileOverlapStat> st;
    if (!DepthNamespace::TileOverlapStats(pmaps, none, g_zenith_range, st)) return 1;
    print("RAW", st);
    if (!DepthNamespace::TileOverlapStats(pmaps, abcd, g_zenith_range, st)) return 1;
    print("FIT", st);
    return 0;
}
