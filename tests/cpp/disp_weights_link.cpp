// A caller of include/pf_depth.h for tests/test_gpu_disp_weights_cli.py: links against
// libpanofuse_depth.so and uses SetDisparityWeights, the facade's extension for per-pixel weights
// of disparity tiles, with MergeDisparityMaps.  A plain build, no sanitizer.
//   disp_weights_link <mode> <arg|-> <width> <baseline_file> <out_file> <tile_file>...
//     SetDisparityWeights(7) must fail ("BADMODE refused"), and SetDisparityWeights(3, "1:0") as
//     well ("BADRANGE refused").  Then SetDisparityWeights(mode, arg) and MergeDisparityMaps of the
//     tile files under the "leres" table's windows into out_file ("MERGED 1"); its "[weights]"
//     lines go to stdout as the facade prints them.  Last, MergeDepthMaps (depth tiles) under the
//     same switch must refuse ("DEPTHTILES refused"), and so must MergeDisparityMaps under
//     SetTileValidity ("WITHRULE refused").
#include "../../include/pf_depth.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

int main(int argc, char** argv)
{
    if (argc < 7) return 2;
    const int mode = std::atoi(argv[1]);
    const std::string arg = std::string(argv[2]) == "-" ? "" : argv[2];
    int width = std::atoi(argv[3]);
    std::string emap_fn(argv[4]), out_fn(argv[5]);
    std::vector<std::string> tile_fns(argv + 6, argv + argc);
    std::vector<Vec4f> fovs, ranges;
    if (!pf_named_layout("leres", fovs, ranges) || fovs.size() != tile_fns.size()) return 1;

    if (DepthNamespace::SetDisparityWeights(7)) return 1;
    std::printf("BADMODE refused\n");
    if (DepthNamespace::SetDisparityWeights(3, "1:0")) return 1;
    std::printf("BADRANGE refused\n");
    std::fflush(stdout);
    if (!DepthNamespace::SetDisparityWeights(mode, arg)) return 1;
    Vec2f zr = g_zenith_range;
    const bool ok = DepthNamespace::MergeDisparityMaps(emap_fn, tile_fns, out_fn, fovs, ranges,
                                                       width, zr, nullptr, nullptr, nullptr,
                                                       nullptr);
    std::printf("MERGED %d\n", ok ? 1 : 0);
    std::fflush(stdout);
    if (!ok) return 1;
    if (mode != 0) {
        std::string again = out_fn + ".depth.png";
        if (DepthNamespace::MergeDepthMaps(emap_fn, tile_fns, again, fovs, ranges, width, zr,
                                           nullptr, nullptr, nullptr, nullptr))
            return 1;
        std::printf("DEPTHTILES refused\n");
        again = out_fn + ".rule.png";
        if (!DepthNamespace::SetTileValidity(true, -INFINITY, INFINITY)) return 1;
        if (DepthNamespace::MergeDisparityMaps(emap_fn, tile_fns, again, fovs, ranges, width, zr,
                                               nullptr, nullptr, nullptr, nullptr))
            return 1;
        std::printf("WITHRULE refused\n");
    }
    return 0;
}
