// pf_depth_mode0.cpp -- the mode-0 driver (Main.cpp:331-687 CreateDepthPanoramas), the RGB tile
// export (Main.cpp:242-326 SaveCubeMap) and the layout entry points of include/pf_depth.h over
// the host-only tables of pf_layouts.cpp.
#include "pf_facade.hpp"
#include "pf_image.hpp"
#include "pf_layouts.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <filesystem>

namespace fs = std::filesystem;
using namespace pff;

// ---- layouts ----
static bool tiles_to_vec4(bool ok, const std::vector<pfl::Tile>& tiles, const std::string& e,
                          std::vector<Vec4f>& fovs, std::vector<Vec4f>& ranges, std::string* err)
{
    if (err) *err = e;
    if (!ok) return false;
    fovs.clear();
    ranges.clear();
    for (const pfl::Tile& t : tiles) {
        fovs.push_back(Vec4f(t.fov[0], t.fov[1], t.fov[2], t.fov[3]));
        ranges.push_back(Vec4f(t.range[0], t.range[1], t.range[2], t.range[3]));
    }
    return true;
}

bool pf_named_layout(const std::string& name, std::vector<Vec4f>& fovs,
                     std::vector<Vec4f>& ranges)
{
    std::vector<pfl::Tile> tiles;
    return tiles_to_vec4(pfl::named(name, tiles), tiles, "", fovs, ranges, nullptr);
}

bool pf_load_layout_file(const std::string& path, std::vector<Vec4f>& fovs,
                         std::vector<Vec4f>& ranges, std::string* err)
{
    std::vector<pfl::Tile> tiles;
    std::string e;
    const bool ok = pfl::load_file(path, tiles, e);
    return tiles_to_vec4(ok, tiles, e, fovs, ranges, err);
}

bool pf_resolve_layout(const std::string& spec, std::vector<Vec4f>& fovs,
                       std::vector<Vec4f>& ranges, std::string* err)
{
    std::vector<pfl::Tile> tiles;
    std::string e;
    const bool ok = pfl::resolve(spec, tiles, e);
    return tiles_to_vec4(ok, tiles, e, fovs, ranges, err);
}

void pf_leres_layout(std::vector<Vec4f>& fovs, std::vector<Vec4f>& ranges)
{
    pf_named_layout("leres", fovs, ranges);  // Main.cpp:788-843, the active "5-fold for LeReS" block
}

namespace {

// The environment switches of mode 0 and of the export (panofuse_main sets them from --layout,
// --edge-metrics, --tile-model), read once at the top of the call.
struct Mode0Switches {
    std::string layout = "leres";  // PF_LAYOUT: a table's name or a layout file
    bool edge_metrics = false;     // PF_EDGE_METRICS=1: <raw>.edges.txt beside .aligned.txt
    bool disparity_tiles = false;  // PF_TILE_MODEL=disparity: MiDaS-style tiles
};

Mode0Switches read_mode0_switches()
{
    Mode0Switches s;
    const char* spec = std::getenv("PF_LAYOUT");
    if (spec && spec[0]) s.layout = spec;
    const char* em = std::getenv("PF_EDGE_METRICS");
    s.edge_metrics = em && em[0] == '1';
    const char* tm = std::getenv("PF_TILE_MODEL");
    s.disparity_tiles = tm && std::string(tm) == "disparity";
    return s;
}

bool resolve_or_print(const std::string& spec, std::vector<Vec4f>& fovs, std::vector<Vec4f>& ranges)
{
    std::string err;
    if (pf_resolve_layout(spec, fovs, ranges, &err)) return true;
    std::cout << "[panofuse] " << err << std::endl;
    return false;
}

// AllFilesInFolder (Main.cpp:50-83): the names of the folder's files (no directories), sorted.
bool list_files(const std::string& folder, std::vector<std::string>& names)
{
    std::error_code ec;
    for (const auto& e : fs::directory_iterator(folder, ec))
        if (!e.is_directory()) names.push_back(e.path().filename().string());
    std::sort(names.begin(), names.end());
    return !ec;
}

std::string join(const std::string& dir, const std::string& name)
{
    return (fs::path(dir) / name).string();
}

std::string raw_name(const std::string& file) { return file.substr(0, file.find_last_of('.')); }

// "<raw>.<a0>_<a1>_<z0>_<z1>." from round(R2D(fov)) (Main.cpp:577-584); the extension follows.
std::string tile_name(const std::string& rawname, const Vec4f& f)
{
    const auto deg = [](float r) { return (int)std::round(r / PF_MYPI_D * 180.0); };
    char name[512];
    std::snprintf(name, sizeof(name), "%s.%d_%d_%d_%d.", rawname.c_str(), deg(f[0]), deg(f[1]),
                  deg(f[2]), deg(f[3]));
    return name;
}

// Mode 0's stand-in for the reference's per-tap "oops!" (Depth.cpp:1595-1604): one line per level
// of the layout the context holds that has taps outside their tile.
void print_layout_audit(pf_ctx* c, int out_width, Vec2f& zr)
{
    int nlevels = 0;
    if (pf_level_info(out_width, out_width / 2, zr[0], zr[1], 0, nullptr, nullptr, nullptr,
                      nullptr, nullptr, &nlevels) != PF_OK)
        return;
    for (int l = 0; l < nlevels; ++l) {
        pf_level_audit a;
        if (!pf_ok(c, pf_layout_audit(c, out_width, out_width / 2, zr[0], zr[1], l, &a),
                   "pf_layout_audit"))
            return;
        if (a.taps_outside > 0)
            std::cout << "[layout] level " << l << " (" << a.w << "x" << a.h << "): "
                      << a.taps_outside << " taps outside their tile (clamped)" << std::endl;
    }
}

// The opt-in edge metrics of mode 0: ErrorLaplacian of the written result and of the baseline
// against the gt, one `name: %f` line per value in the style of Metrics::Save.
bool save_edge_metrics(std::string gt_fn, std::string base_fn, std::string result_fn,
                       const std::string& txt_fn)
{
    EquirectangularMap gt, base, result;
    if (!gt.Load(gt_fn) || !base.Load(base_fn) || !result.Load(result_fn)) return false;
    double g[5], r[5];
    long long ng[3], nr[3];
    if (!DepthNamespace::ErrorLaplacian(gt, base, g[0], g[1], g[2], g[3], g[4], ng) ||
        !DepthNamespace::ErrorLaplacian(gt, result, r[0], r[1], r[2], r[3], r[4], nr))
        return false;
    FILE* fp = std::fopen(txt_fn.c_str(), "w+");
    if (!fp) {
        std::cout << "fopen failed?" << std::endl;
        return false;
    }
    const char* names[5] = {"lap_mse", "lap_mae", "sobelx_mae", "sobely_mae", "lap5_mae"};
    const char* counts[3] = {"n_lap", "n_sobel", "n_lap5"};
    for (int k = 0; k < 5; ++k) {
        std::fprintf(fp, "%s_given: %f\n", names[k], g[k]);
        std::fprintf(fp, "%s_result: %f\n", names[k], r[k]);
    }
    for (int k = 0; k < 3; ++k) {
        std::fprintf(fp, "%s_given: %lld\n", counts[k], ng[k]);
        std::fprintf(fp, "%s_result: %lld\n", counts[k], nr[k]);
    }
    std::fclose(fp);
    return true;
}

// The files of one panorama: the baseline named by the result folder (Main.cpp:499-517), the gt
// (:520-530), the result, and the tiles of the layout (:563-587).
struct PanoFiles {
    std::string base, gt, out;
    std::vector<std::string> tiles;
};

PanoFiles pano_files(const std::string& rawname, const std::string& gt_folder,
                     const std::string& baseline_folder, const std::string& result_folder,
                     const std::string& tile_dir, const std::string& tile_ext,
                     const std::vector<Vec4f>& fovs)
{
    PanoFiles p;
    p.base = join(baseline_folder, rawname + ".jpg");
    if (result_folder.find("Slicenet") != std::string::npos ||
        result_folder.find("slicenet") != std::string::npos)
        p.base = join(baseline_folder, rawname + ".jpg.slicenet.png");
    else if (result_folder.find("unifuse") != std::string::npos)
        p.base = join(baseline_folder, rawname + ".unifuse.jpg");
    else if (result_folder.find("hohonet") != std::string::npos)
        p.base = join(baseline_folder, rawname + ".depth.png");
    p.gt = join(gt_folder, rawname + ".png");
    const size_t k = p.gt.find("_rgb");
    if (k != std::string::npos) p.gt.replace(k, 4, "_depth");
    p.out = join(result_folder, rawname + ".png");
    for (const Vec4f& f : fovs) {
        const std::string name = tile_name(rawname, f);
        std::string fn = join(tile_dir, name + (tile_ext == "auto" ? "jpg" : tile_ext));
        if (tile_ext == "auto" && !fs::exists(fn)) fn = join(tile_dir, name + "png");
        p.tiles.push_back(fn);
    }
    return p;
}

// The averages over the folder (Main.cpp:612-676).
void print_averages(const std::vector<DepthNamespace::Metrics>& all)
{
    double rg = 0, rr = 0, mg = 0, mr = 0, d1g = 0, d1r = 0;
    for (auto& m : all) {
        rg += std::sqrt(m.mse_given);
        rr += std::sqrt(m.mse_result);
        mg += m.mae_given;
        mr += m.mae_result;
        d1g += m.delta1_given;
        d1r += m.delta1_result;
    }
    const double n = (double)all.size();
    std::cout << "RMSE_given:" << rg / n << " RMSE_result:" << rr / n << " MAE_given:" << mg / n
              << " MAE_result_avg:" << mr / n << " delta1_given:" << d1g / n
              << " delta1_result:" << d1r / n << std::endl;
}

}  // namespace

int pf_create_depth_panoramas(const std::string& rgb_folder, const std::string& gt_folder,
                              const std::string& baseline_folder,
                              const std::string& result_folder, const std::string& tile_dir,
                              const std::string& tile_ext, int out_width, int shard,
                              int nshards)
{
    const Mode0Switches sw = read_mode0_switches();
    std::vector<Vec4f> fovs, ranges;
    if (!resolve_or_print(sw.layout, fovs, ranges)) return 2;
    std::vector<std::string> rgb;
    if (!list_files(rgb_folder, rgb)) {
        std::cout << "[CreateDepthPanoramas] cannot list " << rgb_folder << std::endl;
        return 1;
    }
    if (nshards > 1) {  // panorama sharding over processes / GPUs
        std::vector<std::string> mine;
        for (size_t i = (size_t)shard; i < rgb.size(); i += (size_t)nshards) mine.push_back(rgb[i]);
        rgb.swap(mine);
    }
    std::cout << "[CreateDepthPanormas] #RGB_filenames:" << rgb.size() << std::endl;
    bool audited = false;
    std::vector<DepthNamespace::Metrics> all;
    for (size_t i = 0; i < rgb.size(); i++) {
        const std::string rawname = raw_name(rgb[i]);
        PanoFiles f = pano_files(rawname, gt_folder, baseline_folder, result_folder, tile_dir,
                                 tile_ext, fovs);
        if (fs::exists(f.out)) {  // Main.cpp:552-561
            std::cout << i << "/" << rgb.size() << " skip!" << std::endl;
            continue;
        }
        std::cout << i << "/" << rgb.size() << " baseline:" << f.base << std::endl;
        std::cout << "gt:" << f.gt << std::endl << "output_filename:" << f.out << std::endl;
        DepthNamespace::Metrics m;
        int tr = 0, tl = 0;
        const auto merge = sw.disparity_tiles ? DepthNamespace::MergeDisparityMaps
                                              : DepthNamespace::MergeDepthMaps;
        if (!merge(f.base, f.tiles, f.out, fovs, ranges, out_width, g_zenith_range, &f.gt, &m, &tr,
                   &tl)) {
            std::cout << "[CreateDepthPanorma] MergeDepthMaps #" << i << " failed!" << std::endl;
            return 1;
        }
        if (!audited) {  // once: the facade context now holds this layout at this width
            audited = true;
            if (pf_ctx* c = facade_ctx()) print_layout_audit(c, out_width, g_zenith_range);
        }
        m.Save((join(result_folder, rawname) + ".aligned.txt").c_str());
        if (sw.edge_metrics &&
            !save_edge_metrics(f.gt, f.base, f.out, join(result_folder, rawname) + ".edges.txt"))
            std::cout << "[CreateDepthPanorma] no edge metrics for #" << i << std::endl;
        all.push_back(m);
        std::cout << "time_Reg:" << tr << " time_Laplacian:" << tl << std::endl;
    }
    if (!all.empty()) print_averages(all);
    return 0;
}

// ---- RGB tile export (Main.cpp:242-326 SaveCubeMap, called for every panorama by
// CreateDepthPanoramas, Main.cpp:399-430) ----
// Tile size as SaveCubeMap sizes its viewport: width 1024, height round(1024 / aspect) with
// aspect = tan(fovx/2) / tan(fovy/2) (the window-size clamps of a small screen do not apply).
void pff::rgb_tile_size(const Vec4f& f, int& w, int& h)
{
    const float fovx = (float)((f[1] - f[0]) / PF_MYPI_D * 180.0);
    const float fovy = (float)((f[3] - f[2]) / PF_MYPI_D * 180.0);
    const float aspect = (float)(std::tan(PF_D2R(fovx) / 2) / std::tan(PF_D2R(fovy) / 2));
    w = 1024;
    h = (int)std::round((float)w / aspect);
}

// The GL texture of the export is RGB8: gray replicated, alpha dropped, 16-bit reduced to the
// top byte.
static std::vector<uint8_t> to_rgb8(const pfio::Image& im)
{
    std::vector<uint8_t> pano((size_t)im.w * im.h * 3);
    for (size_t p = 0; p < (size_t)im.w * im.h; ++p)
        for (int k = 0; k < 3; ++k) {
            const int ch = im.c >= 3 ? k : 0;
            pano[p * 3 + k] = im.is16 ? (uint8_t)(im.px16[p * im.c + ch] >> 8)
                                      : im.px8[p * im.c + ch];
        }
    return pano;
}

int pf_export_rgb_tiles(const std::string& rgb_folder, const std::string& tile_dir)
{
    const Mode0Switches sw = read_mode0_switches();
    std::vector<Vec4f> fovs, ranges;
    if (!resolve_or_print(sw.layout, fovs, ranges)) return 2;
    pf_ctx* c = facade_ctx();
    if (!c) return 1;
    const int n = (int)fovs.size();
    std::vector<pf_window> fw(n), rw(n);
    std::vector<int> tw(n), th(n);
    size_t total = 0;
    for (int i = 0; i < n; ++i) {
        fw[i] = to_window(fovs[i]);
        rw[i] = to_window(ranges[i]);
        rgb_tile_size(fovs[i], tw[i], th[i]);
        total += (size_t)tw[i] * th[i] * 3;
    }
    if (!pf_ok(c, pf_set_tiles(c, fw.data(), rw.data(), n, tw.data(), th.data(), 1, 1),
               "pf_set_tiles"))
        return 1;
    std::vector<std::string> rgb;
    if (!list_files(rgb_folder, rgb)) {
        std::cout << "[SaveCubeMap] cannot list " << rgb_folder << std::endl;
        return 1;
    }
    std::error_code ec;
    fs::create_directories(tile_dir, ec);
    std::vector<uint8_t> tiles(total);
    for (const std::string& file : rgb) {
        const std::string fn = join(rgb_folder, file);
        pfio::Image im;
        std::string err;
        if (!pfio::load_image(fn, im, err)) {
            std::cout << "[SaveCubeMap] " << err << std::endl;
            return 1;
        }
        const std::vector<uint8_t> pano = to_rgb8(im);
        DevMem dp(pano.data(), pano.size()), dt(total);
        if (!dp.ok || !dt.ok) return 1;
        if (!pf_ok(c, pf_warp_rgb(c, dp.as<uint8_t>(), im.w, im.h, 1, dt.as<uint8_t>()),
                   "pf_warp_rgb") ||
            !download(tiles.data(), dt, total))
            return 1;
        size_t off = 0;
        for (int i = 0; i < n; ++i) {
            // stbi_write_jpg(filename, w, h, 3, data, w * 3): the reference passes the row stride
            // as the quality, which stb clamps to 100 (no chroma subsampling), Main.cpp:319-320
            if (!pfio::save_jpeg(join(tile_dir, tile_name(raw_name(file), fovs[i]) + "jpg"),
                                 tiles.data() + off, tw[i], th[i], 3, tw[i] * 3, err)) {
                std::cout << "[SaveCubeMap] " << err << std::endl;
                return 1;
            }
            off += (size_t)tw[i] * th[i] * 3;
        }
        std::cout << "[SaveCubeMap] " << fn << ": " << n << " tiles" << std::endl;
    }
    return 0;
}
