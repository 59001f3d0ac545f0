// panofuse_main -- the reference's command line (Main.cpp:864-895) for the fusion path:
//   panofuse_main 0 <rgb_dir> <gt_dir> <baseline_dir> <result_dir> [--tiles DIR]
//                 [--ext auto|jpg|png] [--width W] [--device D] [--shard R/N]
//                 [--metrics-order tree|sequential] [--edge-metrics]
//                 [--tile-model depth|disparity] [--global-align] [--layout NAME|FILE]
//                 [--fusion laplacian|smoothing|stitch] [--save-stitch] [--check-laplacian]
//                 [--tile-valid LO:HI] [--reg-loss huber:A|softl1:A] [--tile-depth planar|ray]
//   panofuse_main export <rgb_dir> <tile_dir> [--device D] [--layout NAME|FILE]
//   panofuse_main layout NAME|FILE [--width W] [--tile-size WxH] [--device D]
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
// each RGB panorama becomes the perspective tiles of the chosen layout (by default the 15 LeReS
// tiles) that the depth network consumes.
// --layout: the tile table of mode 0 and of export.  leres (the default: Main.cpp:788-843, the
// reference's active table), midas (:731-787), fold4 (:695-730), fold3 (:845-887), or a layout
// file: one tile per line, eight numbers in degrees (the window's az_left az_right zen_top
// zen_down, then the range's az_left az_right zen_up zen_down), '#' comments; each value becomes
// (float)D2R(deg), computed in double and rounded once.  The tile file names follow the table
// (<raw>.<a0>_<a1>_<z0>_<z1>.<ext> from round(R2D(fov)), Main.cpp:577-584).  A value that is
// neither a known name nor a usable file ends the command with status 2 before any GPU call.
// Mode 0 audits the layout once at its output width and prints, per level that has any,
// "[layout] level L (WxH): N taps outside their tile (clamped)": the reference prints "oops!"
// per such tap and reads past the tile, the library clamps the index.
// "layout" audits a layout on the GPU (pf_layout_audit) at --width (default 2048) with tiles of
// --tile-size (default 1024x1024) and prints, per level,
// "LEVEL l w h h0 h1 outside clamped covered uncovered max_cover seam"; exit 1 with the message
// when pf_set_tiles or the level set-up rejects the layout.
// Mode 0 = CreateDepthPanoramas (Main.cpp:331-687) minus the OpenGL tile export: the perspective
// depth tiles are read from --tiles (default "test_images", the reference's LeReS folder) named
// <raw>.<a0>_<a1>_<z0>_<z1>.<ext>; "auto" takes .jpg when present, else .png (MiDaS naming).
// --metrics-order: the .aligned.txt means in the reference's row-major float order (sequential,
// the default: the digits Main.cpp prints) or in the fp64-tree order (tree: deterministic, within
// 1e-2 relative of the reference's float sums: MEAN_RTOL, the bound tests/test_gpu_metrics.py
// asserts for the tree order).
// --tile-model: what the tiles hold.  depth (the default: LeReS-style tiles, the cubic
// registration) or disparity (MiDaS / DPT tiles, relative inverse depth in 0-1: each is fitted
// with y = 1/(a x + b) + d and mapped to depth by D2DTransform).  The reference's MiDaS folder
// convention (Main.cpp:577-579) is `--layout midas --tiles output --ext png`.
// --global-align (opt-in, takes no value): after the fusion the u16 result is registered to the
// baseline with SolveDepthToDepth2's cubic (Depth.cpp:1158-1259) and transformed, before it is
// written and scored; prints the "[SolveDepthToDepth2] ..." line per panorama.
// --edge-metrics (opt-in, takes no value): also write <raw>.edges.txt per panorama, the
// ErrorLaplacian values of the result and of the baseline against the gt.
// --fusion laplacian|smoothing|stitch: what fills the result (Depth.cpp:904-922, :851).  laplacian
// (the default) is SolveDepthAll; smoothing is SolveDepthBySmoothing and stitch the direct tile
// stitch (Depth.cpp:817-865), both on the registered tiles.  Everything after it (the result file,
// the metrics, the masks, --global-align, --edge-metrics) runs on that result.
// --save-stitch (opt-in, takes no value): also write <raw>.png.pmap.png, the direct stitch of the
// registered tiles (the reference's debug file, Depth.cpp:859).
// --check-laplacian (opt-in, takes no value, only with --fusion laplacian): print SolveDepthAll's
// self-check "[SolveDepthAll] check Laplacian err:<err>" (Depth.cpp:1738-1758) per panorama.
// --tile-valid LO:HI (opt-in): the tile-pixel validity rule (pf_set_tile_validity).  A tile pixel
// is read as depth only if LO < v < HI, v being the file's value after it is scaled to 0..1; LO
// and HI are floats, "-inf" and "inf" included (0:inf skips black bars and holes written as 0,
// 0:1 saturated pixels as well).  Registration, fusion and stitch skip the others, and the run
// prints "[mask] tile <i>: <n> of <N> pixels invalid, <m> of <M> samples" per tile that has any.
// Not with --tile-model disparity or --fusion smoothing.  Carried in PF_TILE_VALID.  (The usage
// text of the bare command is pinned by the tests and does not list it.)
// --reg-loss huber:A|softl1:A (opt-in): the tile registrations run under Ceres' HuberLoss(A) or
// SoftLOneLoss(A) (pf_set_register_loss), and the run prints per tile "[robust] tile <i>: <m> of
// <n> samples beyond a=<A>, cost <c0> -> <c1>, <it> iterations, <termination>".  Not with
// --global-align.  Carried in PF_REG_LOSS; not in the usage text either.
// --tile-depth planar|ray (opt-in): what the tiles hold (pf_set_tile_depth).  ray (the default) is
// distance from the camera centre, as the reference assumes; planar is depth along the optical
// axis, what perspective depth networks predict.  Under planar the registration fits the tile
// model times the pixel's ray factor and transforms the uploaded tiles, --fusion, --save-stitch and
// --check-laplacian run on those without coefficients, and the run prints per panorama
// "[tile-depth] planar: ray factor up to <max> over <n> tiles".  Works with both --tile-model
// values.  Carried in PF_TILE_DEPTH; not in the usage text either.
// --reg-consistent LAMBDA (opt-in): the tiles are registered together instead of one by one, each to
// the baseline and to its neighbours where their windows overlap, LAMBDA >= 0 weighing the overlap
// term (pf_register_consistent); the fusion, stitch or smoothing then runs as ever.  Prints per
// panorama "[consistent] lambda <L>: <P> pairs, <S> pair samples, overlap rms <before> -> <after>".
// Not with --tile-model disparity or --global-align (refused here), nor with --tile-valid,
// --reg-loss or --tile-depth planar (refused with the library's message).  Carried in
// PF_REG_CONSISTENT; not in the usage text either.
// --tile-weights tent|files:SUFFIX (opt-in): per-pixel tile weights (pf_register_weighted,
// pf_fuse_weighted).  tent is the blending tent of every tile; with files:SUFFIX the weight map of a
// tile file F is F + SUFFIX (a PNG in 0-1 or a PFM of the tile's size, else the run names the file
// and fails).  A weight outside (0, +inf) switches its pixel off.  The run prints per tile
// "[weights] tile <i>: <n> of <N> samples used, sum w <s>".  Not with --tile-valid, --reg-loss,
// --tile-depth planar, --reg-consistent, --tile-model disparity, --global-align, --check-laplacian
// or --fusion smoothing|stitch (refused here).  Carried in PF_TILE_WEIGHTS; not in the usage text
// either.
// --disparity-weights tent|files:SUFFIX|range:LO:HI (opt-in, with --tile-model disparity): per-pixel
// weights for disparity tiles (pf_register_disparity_weighted, pf_merge_disparity_weighted).  tent
// and files:SUFFIX as --tile-weights'; range:LO:HI counts a pixel iff LO < v < HI (range:0:inf
// drops the disparity-0 sky a network writes).  Prints --tile-weights' "[weights]" lines.  Works
// with --tile-depth planar.  Not without --tile-model disparity, nor with --tile-valid, --reg-loss,
// --reg-consistent, --global-align, --check-laplacian, --fusion smoothing|stitch or --tile-weights
// (refused here).  Carried in PF_DISPARITY_WEIGHTS; not in the usage text either.
#include "pf_disp_weights.hpp"
#include "pf_facade.hpp"  // the inline to_window and load_pair; it includes the two public headers
#include "pf_ray.hpp"
#include "pf_valid.hpp"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using pff::to_window;

static const char* const kUsageExport = " export <rgb_dir> <tile_dir> [--device D] [--layout NAME|FILE]";
static const char* const kUsageLayout = " layout NAME|FILE [--width W] [--tile-size WxH] [--device D]";
static const char* const kUsageLap = " lap <gt_file> <given_file> [--device D]";
static const char* const kUsageCmp =
    " cmp <gt_file> <given_file> [--disp] [--align 0|1|2] [--no-cap] [--save FILE] [--device D]"
    " [--metrics-order tree|sequential]";

static int usage(const char* argv0, const char* text)
{
    std::cout << "usage: " << argv0 << text << std::endl;
    return 1;
}

// The answer to a rejected option value, and its exit status.
static int bad(const std::string& k, const std::string& v, const std::string& want)
{
    std::cout << "bad " << k << " " << v << " (want " << want << ")" << std::endl;
    return 2;
}

static bool select_device(int dev)
{
    if (hipSetDevice(dev) == hipSuccess) return true;
    std::cout << "no HIP device " << dev << std::endl;
    return false;
}

// An option that travels to the facade in an environment variable: a switch (no values: the
// variable becomes "1") or one of the listed values.
struct EnvFlag {
    const char* name;
    std::vector<const char*> values;
    const char* var;
};
static const EnvFlag kEnvFlags[] = {
    {"--edge-metrics", {}, "PF_EDGE_METRICS"},  // read by pf_create_depth_panoramas
    {"--tile-model", {"depth", "disparity"}, "PF_TILE_MODEL"},
    {"--global-align", {}, "PF_GLOBAL_ALIGN"},  // read by MergeDepthMaps / MergeDisparityMaps
    {"--save-stitch", {}, "PF_SAVE_STITCH"},
    {"--check-laplacian", {}, "PF_CHECK_LAPLACIAN"},
    {"--fusion", {"laplacian", "smoothing", "stitch"}, "PF_FUSION"},
    {"--metrics-order", {"tree", "sequential"}, "PF_METRICS_ORDER"},  // when the context is made
};

// The handlers below answer 0 (taken), 2 (rejected, the message is printed) or -1 (not mine).
// k as a switch (v null) or with its value v.
static int take_env_flag(const std::string& k, const char* v)
{
    for (const EnvFlag& f : kEnvFlags) {
        if (k != f.name || f.values.empty() != !v) continue;
        bool ok = !v;
        std::string want;  // "a, b or c"
        for (size_t i = 0; i < f.values.size(); ++i) {
            ok = ok || std::string(f.values[i]) == v;
            want += i == 0 ? "" : i + 1 == f.values.size() ? " or " : ", ";
            want += f.values[i];
        }
        if (!ok) return bad(k, v, want);
        setenv(f.var, v ? v : "1", 1);
        return 0;
    }
    return -1;
}

// --layout's value: checked here (no GPU call yet), carried to the facade in PF_LAYOUT.
static int take_layout(const std::string& v)
{
    std::vector<Vec4f> fovs, ranges;
    std::string err;
    if (!pf_resolve_layout(v, fovs, ranges, &err)) {
        std::cout << "bad --layout: " << err << std::endl;
        return 2;
    }
    setenv("PF_LAYOUT", v.c_str(), 1);  // read by pf_create_depth_panoramas / pf_export_rgb_tiles
    return 0;
}

// Walks argv[first..]: on_switch(k) takes an option that has no value, on_value(k, v) one that
// has.  An option at the end that lacks its value ends the walk: silently when `lenient` (mode 0),
// else with "option ... needs a value" and status 2.  Returns 0 or the status to exit with.
template <class OnSwitch, class OnValue>
static int walk_options(int argc, char* argv[], int first, bool lenient, OnSwitch on_switch,
                        OnValue on_value)
{
    for (int i = first; i < argc; ++i) {
        const std::string k(argv[i]);
        int rc = on_switch(k);
        if (rc < 0) {
            if (i + 1 >= argc) {
                if (lenient) break;
                std::cout << "option " << k << " needs a value" << std::endl;
                return 2;
            }
            rc = on_value(k, std::string(argv[++i]));
            if (rc < 0) {
                std::cout << "unknown option " << k << std::endl;
                return 2;
            }
        }
        if (rc > 0) return rc;
    }
    return 0;
}

static int no_switch(const std::string&) { return -1; }

static int layout_command(int argc, char* argv[])
{
    if (argc < 3) return usage(argv[0], kUsageLayout);
    int width = 2048, tw = 1024, th = 1024, dev = 0;
    const auto on_value = [&](const std::string& k, const std::string& v) {
        if (k == "--width") width = std::atoi(v.c_str());
        else if (k == "--device") dev = std::atoi(v.c_str());
        else if (k != "--tile-size") return -1;
        else if (std::sscanf(v.c_str(), "%dx%d", &tw, &th) != 2 || tw < 2 || th < 2)
            return bad(k, v, "WxH");
        return 0;
    };
    if (int rc = walk_options(argc, argv, 3, false, no_switch, on_value)) return rc;
    std::vector<Vec4f> fovs, ranges;
    std::string err;
    if (!pf_resolve_layout(argv[2], fovs, ranges, &err)) {
        std::cout << "bad layout: " << err << std::endl;
        return 2;
    }
    if (!select_device(dev)) return 1;
    pf_ctx* c = nullptr;
    if (pf_create(dev, &c) != PF_OK) {
        std::cout << "pf_create(" << dev << ") failed" << std::endl;
        return 1;
    }
    const int n = (int)fovs.size();
    std::vector<pf_window> fw(n), rw(n);
    std::vector<int> tws(n, tw), ths(n, th);
    for (int i = 0; i < n; ++i) {
        fw[i] = to_window(fovs[i]);
        rw[i] = to_window(ranges[i]);
    }
    int rc = pf_set_tiles(c, fw.data(), rw.data(), n, tws.data(), ths.data(), 1, 1);
    int nlevels = 0;
    if (rc == PF_OK)
        rc = pf_level_info(width, width / 2, g_zenith_range[0], g_zenith_range[1], 0, nullptr,
                           nullptr, nullptr, nullptr, nullptr, &nlevels);
    for (int l = 0; rc == PF_OK && l < nlevels; ++l) {
        pf_level_audit a;
        rc = pf_layout_audit(c, width, width / 2, g_zenith_range[0], g_zenith_range[1], l, &a);
        if (rc == PF_OK)
            std::printf("LEVEL %d %d %d %d %d %lld %lld %lld %lld %d %d\n", l, a.w, a.h, a.h0, a.h1,
                        a.taps_outside, a.taps_clamped, a.covered, a.uncovered_interior,
                        a.max_cover, a.seam);
    }
    if (rc != PF_OK) {
        const char* msg = pf_last_error(c);
        std::cout << "layout rejected (" << rc << "): "
                  << (msg && msg[0] ? msg : "bad output width") << std::endl;
    }
    std::fflush(stdout);
    pf_destroy(c);
    return rc == PF_OK ? 0 : 1;
}

static int export_command(int argc, char* argv[])
{
    if (argc < 4) return usage(argv[0], kUsageExport);
    int dev = 0;
    const auto on_value = [&](const std::string& k, const std::string& v) {
        if (k == "--layout") return take_layout(v);
        if (k != "--device") return -1;
        dev = std::atoi(v.c_str());
        return 0;
    };
    if (int rc = walk_options(argc, argv, 4, false, no_switch, on_value)) return rc;
    if (!select_device(dev)) return 1;
    return pf_export_rgb_tiles(argv[2], argv[3]);
}

static int lap_command(int argc, char* argv[])
{
    if (argc < 4) return usage(argv[0], kUsageLap);
    // --device is taken as the fourth argument only
    const int dev = argc >= 6 && std::string(argv[4]) == "--device" ? std::atoi(argv[5]) : 0;
    if (!select_device(dev)) return 1;
    std::string gt_fn(argv[2]), given_fn(argv[3]);
    DepthNamespace::EquirectangularMap gt, given;
    if (!pff::load_pair(gt_fn, given_fn, false, gt, given)) return 1;
    double v[5];
    long long n[3];
    if (!DepthNamespace::ErrorLaplacian(gt, given, v[0], v[1], v[2], v[3], v[4], n)) return 1;
    std::cout << "[ErrorLap] n_lap:" << n[0] << " n_sobel:" << n[1] << " n_lap5:" << n[2]
              << std::endl;
    return 0;
}

static int cmp_command(int argc, char* argv[])
{
    if (argc < 4) return usage(argv[0], kUsageCmp);
    bool disp = false, cap = true;
    int align = 1, dev = 0;
    std::string save;
    const auto on_switch = [&](const std::string& k) {
        if (k == "--disp") disp = true;
        else if (k == "--no-cap") cap = false;
        else return -1;
        return 0;
    };
    const auto on_value = [&](const std::string& k, const std::string& v) {
        if (k == "--align") align = std::atoi(v.c_str());
        else if (k == "--save") save = v;
        else if (k == "--device") dev = std::atoi(v.c_str());
        else if (k == "--metrics-order") return take_env_flag(k, v.c_str());
        else return -1;
        return 0;
    };
    if (int rc = walk_options(argc, argv, 4, false, on_switch, on_value)) return rc;
    if (align < 0 || align > 2) return bad("--align", std::to_string(align), "0, 1 or 2");
    // the loads come first: a file that does not load ends the command before any GPU call
    std::string gt_fn(argv[2]), given_fn(argv[3]);
    DepthNamespace::EquirectangularMap gt, given;
    if (!pff::load_pair(gt_fn, given_fn, true /*mono360*/, gt, given)) return 1;
    if (!select_device(dev)) return 1;
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

static int mode0_command(int argc, char* argv[])
{
    if (argc < 6) {
        std::cout << "[CreateDepthPanormas] error: need argc>=6" << std::endl;
        return 1;
    }
    std::string tiles = "test_images", ext = "auto", fusion;
    int width = 2048, device = 0, shard = 0, nshards = 1;
    bool check_laplacian = false, consistent = false, global_align = false, disparity = false;
    bool weights = false, planar = false, tile_valid = false, reg_loss = false;
    bool disp_weights = false;
    const auto on_switch = [&](const std::string& k) {
        if (k == "--check-laplacian") check_laplacian = true;
        if (k == "--global-align") global_align = true;
        return take_env_flag(k, nullptr);
    };
    const auto on_value = [&](const std::string& k, const std::string& v) {
        if (k == "--tiles") tiles = v;
        else if (k == "--ext") ext = v;
        else if (k == "--width") width = std::atoi(v.c_str());
        else if (k == "--device") device = std::atoi(v.c_str());
        else if (k == "--layout") return take_layout(v);
        else if (k == "--tile-valid") {
            float lo, hi;
            std::string err;
            if (!pfv::parse_range(v.c_str(), lo, hi, err)) return bad(k, v, "LO:HI, LO < HI");
            tile_valid = true;
            setenv("PF_TILE_VALID", v.c_str(), 1);  // read by MergeDepthMaps
        }
        else if (k == "--reg-loss") {
            pff::RegLossRule r;
            if (!pff::parse_reg_loss(v.c_str(), r)) return bad(k, v, "huber:A or softl1:A, A > 0");
            reg_loss = true;
            setenv("PF_REG_LOSS", v.c_str(), 1);  // read by MergeDepthMaps / MergeDisparityMaps
        }
        else if (k == "--tile-depth") {
            if (pf::parse_tile_depth(v.c_str()) < 0) return bad(k, v, "planar or ray");
            planar = v == "planar";
            setenv("PF_TILE_DEPTH", v.c_str(), 1);  // read by MergeDepthMaps / MergeDisparityMaps
        }
        else if (k == "--reg-consistent") {
            char* end = nullptr;
            const double lam = std::strtod(v.c_str(), &end);
            if (v.empty() || !end || *end != '\0' || !(lam >= 0.0 && lam < HUGE_VAL))
                return bad(k, v, "a finite LAMBDA >= 0");
            consistent = true;
            setenv("PF_REG_CONSISTENT", v.c_str(), 1);  // read by MergeDepthMaps
        }
        else if (k == "--tile-weights") {
            pfw::Spec spec;
            std::string err;
            if (!pfw::parse_spec(v.c_str(), spec, err) || spec.mode == pfw::OFF)
                return bad(k, v, "tent or files:SUFFIX");
            weights = true;
            setenv("PF_TILE_WEIGHTS", v.c_str(), 1);  // read by MergeDepthMaps
        }
        else if (k == "--disparity-weights") {
            pfdw::Spec spec;
            std::string err;
            if (!pfdw::parse_spec(v.c_str(), spec, err) || spec.mode == pfdw::OFF)
                return bad(k, v, "tent, files:SUFFIX or range:LO:HI");
            disp_weights = true;
            setenv("PF_DISPARITY_WEIGHTS", v.c_str(), 1);  // read by MergeDisparityMaps
        }
        else if (k == "--shard") {  // R/N: one process per GPU over the sorted folder
            if (std::sscanf(v.c_str(), "%d/%d", &shard, &nshards) != 2 || nshards < 1 ||
                shard < 0 || shard >= nshards)
                return bad(k, v, "R/N, 0 <= R < N");
        }
        else {
            if (k == "--fusion") fusion = v;
            if (k == "--tile-model") disparity = v == "disparity";
            return take_env_flag(k, v.c_str());
        }
        return 0;
    };
    if (int rc = walk_options(argc, argv, 6, true, on_switch, on_value)) return rc;
    // the self-check compares the Jacobi result with its targets: only the fusion has them.  The
    // facade has the same rule for its environment; this one fails before any GPU call.
    if (check_laplacian && !fusion.empty() && fusion != "laplacian") {
        std::cout << "--check-laplacian needs --fusion laplacian (got " << fusion << ")"
                  << std::endl;
        return 2;
    }
    if (disp_weights) {  // the weighted disparity forms stand alone: refused before any GPU call
        pfdw::Others o;
        o.disparity_tiles = disparity;
        o.tile_valid = tile_valid;
        o.reg_loss = reg_loss;
        o.consistent = consistent;
        o.global_align = global_align;
        o.check_laplacian = check_laplacian;
        o.tile_weights = weights;
        o.smoothing = fusion == "smoothing";
        o.stitch = fusion == "stitch";
        if (const char* what = pfdw::clash(o, true)) {
            std::cout << pfdw::clash_message(what, true) << std::endl;
            return 2;
        }
    }
    if (consistent && (disparity || global_align)) {
        std::cout << "--reg-consistent registers depth tiles by a linear solve: not with "
                  << (disparity ? "--tile-model disparity" : "--global-align") << std::endl;
        return 2;
    }
    if (weights) {  // the weighted forms stand alone: refused before any GPU call
        const char* clash = tile_valid              ? "--tile-valid"
                            : reg_loss              ? "--reg-loss"
                            : planar                ? "--tile-depth planar"
                            : consistent            ? "--reg-consistent"
                            : disparity             ? "--tile-model disparity"
                            : global_align          ? "--global-align"
                            : fusion == "smoothing" ? "--fusion smoothing"
                            : fusion == "stitch"    ? "--fusion stitch"
                            : check_laplacian       ? "--check-laplacian"
                                                    : nullptr;
        if (clash) {
            std::cout << "--tile-weights registers and fuses with per-pixel weights: not with "
                      << clash << std::endl;
            return 2;
        }
    }
    if (!select_device(device)) return 1;
    return pf_create_depth_panoramas(argv[2], argv[3], argv[4], argv[5], tiles, ext, width, shard,
                                     nshards);
}

int main(int argc, char* argv[])
{
    if (argc < 2) {
        std::cout << "usage: " << argv[0]
                  << " 0 <rgb_dir> <gt_dir> <baseline_dir> <result_dir> [--tiles DIR]"
                     " [--ext auto|jpg|png] [--width W] [--device D] [--shard R/N]"
                     " [--metrics-order tree|sequential] [--edge-metrics]"
                     " [--tile-model depth|disparity] [--global-align] [--layout NAME|FILE]"
                     " [--fusion laplacian|smoothing|stitch] [--save-stitch]"
                     " [--check-laplacian]\n"
                     "         (MiDaS disparity tiles, the reference's folder convention:"
                     " --layout midas --tile-model disparity --tiles output --ext png)\n"
                     "         (--layout: leres (default), midas, fold4, fold3, or a file of"
                     " lines `faz0 faz1 fzen0 fzen1 raz0 raz1 rzen0 rzen1` in degrees)\n       "
                  << argv[0] << kUsageExport << "\n       " << argv[0] << kUsageLayout
                  << "\n       " << argv[0] << kUsageLap << "\n       " << argv[0] << kUsageCmp
                  << std::endl;
        return 0;
    }
    const std::string cmd(argv[1]);
    if (cmd == "export") return export_command(argc, argv);
    if (cmd == "layout") return layout_command(argc, argv);
    if (cmd == "lap") return lap_command(argc, argv);
    if (cmd == "cmp") return cmp_command(argc, argv);
    if (cmd == "0") return mode0_command(argc, argv);
    return 0;  // Main.cpp:889-893: other commands do nothing
}
