// panofuse_main -- the reference's command line (Main.cpp:864-895) for the fusion path:
//   panofuse_main 0 <rgb_dir> <gt_dir> <baseline_dir> <result_dir> [--tiles DIR]
//                 [--ext auto|jpg|png] [--width W] [--device D] [--shard R/N]
//                 [--metrics-order tree|sequential] [--edge-metrics]
//                 [--tile-model depth|disparity] [--global-align]
//   panofuse_main export <rgb_dir> <tile_dir> [--device D]
//   panofuse_main lap <gt_file> <given_file> [--device D]
//   panofuse_main cmp <gt_file> <given_file> [--disp] [--align 0|1|2] [--no-cap] [--save FILE]
//                 [--device D] [--metrics-order tree|sequential]
// "cmp" is the reference's ErrorCompare (Depth.cpp:2460-2634) on two image files, the given one
// loaded the mono360 way: depth against depth by default (align 1, cap on), with --disp the given
// map is a disparity that is least-squares-aligned to the gt's first.  It prints
// "CMP mse mae mre mselog delta1 delta2 delta3" at %.9g, with --disp also
// "FIT s o vmin vmax n_nonblack", and with --save writes the 8-bit PNG the reference saves.
// "lap" is the reference's ErrorLaplacian (Depth.cpp:2636-2953) on two image files: its
// "[ErrorLap] ..." line, then one line with the three sample counts.
// "export" is the tile render of mode 0 (Main.cpp:399-430, SaveCubeMap :242-326) on the GPU:
// each RGB panorama becomes the 15 LeReS perspective tiles the depth network consumes.
// Mode 0 = CreateDepthPanoramas (Main.cpp:331-687) minus the OpenGL tile export: the perspective
// depth tiles are read from --tiles (default "test_images", the reference's LeReS folder) named
// <raw>.<a0>_<a1>_<z0>_<z1>.<ext>; "auto" takes .jpg when present, else .png (MiDaS naming).
// --metrics-order: the .aligned.txt means in the reference's row-major float order (sequential,
// the default: the digits Main.cpp prints) or in the fp64-tree order (tree: deterministic, within
// ~1e-3 relative of the reference's float sums).
// --tile-model: what the tiles hold.  depth (the default: LeReS-style tiles, the cubic
// registration) or disparity (MiDaS / DPT tiles, relative inverse depth in 0-1: each is fitted
// with y = 1/(a x + b) + d and mapped to depth by D2DTransform).  The reference's MiDaS folder
// convention (Main.cpp:577-579) is `--tiles output --ext png`.
// --global-align (opt-in, takes no value): after the fusion the u16 result is registered to the
// baseline with SolveDepthToDepth2's cubic (Depth.cpp:1158-1259) and transformed, before it is
// written and scored; prints the "[SolveDepthToDepth2] ..." line per panorama.
// --edge-metrics (opt-in, takes no value): also write <raw>.edges.txt per panorama, the
// ErrorLaplacian values of the result and of the baseline against the gt.
#include "../../include/pf_depth.h"

#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

int main(int argc, char* argv[])
{
    if (argc < 2) {
        std::cout << "usage: " << argv[0]
                  << " 0 <rgb_dir> <gt_dir> <baseline_dir> <result_dir> [--tiles DIR]"
                     " [--ext auto|jpg|png] [--width W] [--device D] [--shard R/N]"
                     " [--metrics-order tree|sequential] [--edge-metrics]"
                     " [--tile-model depth|disparity] [--global-align]\n"
                     "         (MiDaS disparity tiles, the reference's folder convention:"
                     " --tile-model disparity --tiles output --ext png)\n       "
                  << argv[0] << " export <rgb_dir> <tile_dir> [--device D]\n       "
                  << argv[0] << " lap <gt_file> <given_file> [--device D]\n       "
                  << argv[0]
                  << " cmp <gt_file> <given_file> [--disp] [--align 0|1|2] [--no-cap] [--save FILE]"
                     " [--device D] [--metrics-order tree|sequential]"
                  << std::endl;
        return 0;
    }
    const std::string cmd(argv[1]);
    if (cmd == "export") {
        if (argc < 4) {
            std::cout << "usage: " << argv[0] << " export <rgb_dir> <tile_dir> [--device D]"
                      << std::endl;
            return 1;
        }
        const int dev = argc >= 6 && std::string(argv[4]) == "--device" ? std::atoi(argv[5]) : 0;
        if (hipSetDevice(dev) != hipSuccess) {
            std::cout << "no HIP device " << dev << std::endl;
            return 1;
        }
        return pf_export_rgb_tiles(argv[2], argv[3]);
    }
    if (cmd == "lap") {
        if (argc < 4) {
            std::cout << "usage: " << argv[0] << " lap <gt_file> <given_file> [--device D]"
                      << std::endl;
            return 1;
        }
        const int dev = argc >= 6 && std::string(argv[4]) == "--device" ? std::atoi(argv[5]) : 0;
        if (hipSetDevice(dev) != hipSuccess) {
            std::cout << "no HIP device " << dev << std::endl;
            return 1;
        }
        std::string gt_fn(argv[2]), given_fn(argv[3]);
        DepthNamespace::EquirectangularMap gt, given;
        if (!gt.Load(gt_fn)) {
            std::cout << "cannot load emap_gt? " << gt_fn << std::endl;
            return 1;
        }
        if (!given.Load(given_fn)) {
            std::cout << "cannot load emap_baseline? " << given_fn << std::endl;
            return 1;
        }
        double v[5];
        long long n[3];
        if (!DepthNamespace::ErrorLaplacian(gt, given, v[0], v[1], v[2], v[3], v[4], n)) return 1;
        std::cout << "[ErrorLap] n_lap:" << n[0] << " n_sobel:" << n[1] << " n_lap5:" << n[2]
                  << std::endl;
        return 0;
    }
    if (cmd == "cmp") {
        if (argc < 4) {
            std::cout << "usage: " << argv[0]
                      << " cmp <gt_file> <given_file> [--disp] [--align 0|1|2] [--no-cap]"
                         " [--save FILE] [--device D] [--metrics-order tree|sequential]"
                      << std::endl;
            return 1;
        }
        bool disp = false, cap = true;
        int align = 1, dev = 0;
        std::string save;
        for (int i = 4; i < argc; ++i) {
            const std::string k(argv[i]);
            if (k == "--disp") disp = true;
            else if (k == "--no-cap") cap = false;
            else if (i + 1 >= argc) {
                std::cout << "option " << k << " needs a value" << std::endl;
                return 2;
            }
            else if (k == "--align") align = std::atoi(argv[++i]);
            else if (k == "--save") save = argv[++i];
            else if (k == "--device") dev = std::atoi(argv[++i]);
            else if (k == "--metrics-order") {
                const std::string v(argv[++i]);
                if (v != "tree" && v != "sequential") {
                    std::cout << "bad --metrics-order " << v << " (want tree or sequential)"
                              << std::endl;
                    return 2;
                }
                setenv("PF_METRICS_ORDER", v.c_str(), 1);  // read when the facade's context is made
            }
            else {
                std::cout << "unknown option " << k << std::endl;
                return 2;
            }
        }
        if (align < 0 || align > 2) {
            std::cout << "bad --align " << align << " (want 0, 1 or 2)" << std::endl;
            return 2;
        }
        // the loads come first: a file that does not load ends the command before any GPU call
        std::string gt_fn(argv[2]), given_fn(argv[3]);
        DepthNamespace::EquirectangularMap gt, given;
        if (!gt.Load(gt_fn)) {
            std::cout << "cannot load emap_gt? " << gt_fn << std::endl;
            return 1;
        }
        if (!given.Load(given_fn, true /*mono360*/)) {
            std::cout << "cannot load emap_baseline? " << given_fn << std::endl;
            return 1;
        }
        if (hipSetDevice(dev) != hipSuccess) {
            std::cout << "no HIP device " << dev << std::endl;
            return 1;
        }
        float v[7];
        Vec2f fit, minmax;
        int n_nonblack = 0;
        std::vector<unsigned char> shifted;
        if (!DepthNamespace::ErrorCompare(gt, given, disp, v[0], v[1], v[2], v[3], v[4], v[5], v[6],
                                          align, cap, &fit, &minmax, save.empty() ? nullptr : &shifted,
                                          &n_nonblack))
            return 1;
        std::printf("CMP %.9g %.9g %.9g %.9g %.9g %.9g %.9g\n", v[0], v[1], v[2], v[3], v[4], v[5],
                    v[6]);
        if (disp)
            std::printf("FIT %.9g %.9g %.9g %.9g %d\n", fit[0], fit[1], minmax[0], minmax[1],
                        n_nonblack);
        std::fflush(stdout);
        if (!save.empty()) {
            const bool ok = Save8BitPNG(shifted.data(), given.width, given.height, save.c_str());
            std::cout << "[ErrorCompare] " << (ok ? 1 : 0) << " saved shifted emap:" << save
                      << std::endl;
            if (!ok) return 1;
        }
        return 0;
    }
    if (cmd != "0") return 0;  // Main.cpp:889-893: other commands do nothing
    if (argc < 6) {
        std::cout << "[CreateDepthPanormas] error: need argc>=6" << std::endl;
        return 1;
    }
    std::string tiles = "test_images", ext = "auto";
    int width = 2048, device = 0, shard = 0, nshards = 1;
    for (int i = 6; i < argc; i += 2) {
        const std::string k(argv[i]);
        if (k == "--edge-metrics") {  // a flag without a value
            setenv("PF_EDGE_METRICS", "1", 1);  // read by pf_create_depth_panoramas
            --i;
            continue;
        }
        if (k == "--global-align") {  // a flag without a value
            setenv("PF_GLOBAL_ALIGN", "1", 1);  // read by MergeDepthMaps / MergeDisparityMaps
            --i;
            continue;
        }
        if (i + 1 >= argc) break;
        const std::string v(argv[i + 1]);
        if (k == "--tiles") tiles = v;
        else if (k == "--ext") ext = v;
        else if (k == "--width") width = std::atoi(v.c_str());
        else if (k == "--device") device = std::atoi(v.c_str());
        else if (k == "--metrics-order") {
            if (v != "tree" && v != "sequential") {
                std::cout << "bad --metrics-order " << v << " (want tree or sequential)" << std::endl;
                return 2;
            }
            setenv("PF_METRICS_ORDER", v.c_str(), 1);  // read when the facade's context is made
        }
        else if (k == "--tile-model") {
            if (v != "depth" && v != "disparity") {
                std::cout << "bad --tile-model " << v << " (want depth or disparity)" << std::endl;
                return 2;
            }
            setenv("PF_TILE_MODEL", v.c_str(), 1);  // read by pf_create_depth_panoramas
        }
        else if (k == "--shard") {  // R/N: one process per GPU over the sorted folder
            if (std::sscanf(v.c_str(), "%d/%d", &shard, &nshards) != 2 || nshards < 1 ||
                shard < 0 || shard >= nshards) {
                std::cout << "bad --shard " << v << " (want R/N, 0 <= R < N)" << std::endl;
                return 2;
            }
        }
        else {
            std::cout << "unknown option " << k << std::endl;
            return 2;
        }
    }
    if (hipSetDevice(device) != hipSuccess) {
        std::cout << "no HIP device " << device << std::endl;
        return 1;
    }
    return pf_create_depth_panoramas(argv[2], argv[3], argv[4], argv[5], tiles, ext, width, shard,
                                     nshards);
}
