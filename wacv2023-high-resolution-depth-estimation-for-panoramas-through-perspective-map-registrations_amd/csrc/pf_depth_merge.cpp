// pf_depth_merge.cpp -- MergeDepthMaps and MergeDisparityMaps of the DepthNamespace facade.
//
// The reference's MergeDepthMaps (Depth.cpp:754-1041) loads the baseline and the tiles, runs
// SolveDepthToDepth + Depth2DepthTransform per tile, SolveDepthAll, writes the u16 PNG and, with
// a ground truth, ErrorEmap/ErrorData plus the .res.png/.giv.png masks.  Here the loads and the
// file writes stay on the host (they are file formats), every per-pixel computation of the path
// (registration, transform, fusion, quantisation, metrics) is a libpanofuse HIP kernel.
#include "pf_disp_weights.hpp"
#include "pf_facade.hpp"
#include "pf_image.hpp"
#include "pf_ray.hpp"
#include "pf_valid.hpp"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <future>

namespace DepthNamespace {
namespace {
using namespace pff;

// The environment switches of a Merge* call (panofuse_main sets them from --fusion,
// --save-stitch, --check-laplacian, --global-align, --reg-consistent), read once at the top of the
// call.
// fusion: what fills the result (Depth.cpp:904-922, :851), the choice the reference makes by
// editing `if (true/false)`; save_stitch / check_laplacian: its two `if (false)` diagnostics
// (:817-865, :1738-1758); global_align: the fused result is pulled back onto the baseline by
// SolveDepthToDepth2's cubic before it is written and scored.
struct MergeSwitches {
    enum { LAPLACIAN, SMOOTHING, STITCH } fusion = LAPLACIAN;
    bool save_stitch = false, check_laplacian = false, global_align = false;
    // PF_TILE_VALID=LO:HI (panofuse_main --tile-valid): the tile-pixel validity rule of this
    // call; without it the rule is SetTileValidity's
    TileRule rule{false, 0.0f, 0.0f};
    // PF_REG_LOSS=huber:A|softl1:A (panofuse_main --reg-loss): the registration loss of this
    // call; without it the loss is SetRegistrationLoss's
    RegLossRule loss{PF_LOSS_NONE, 0.0};
    // PF_TILE_DEPTH=planar|ray (panofuse_main --tile-depth): what the tiles of this call hold;
    // without it SetTileDepth's
    int tile_depth = PF_TILE_DEPTH_RAY;
    // PF_REG_CONSISTENT=LAMBDA (panofuse_main --reg-consistent): the tiles are registered together,
    // to the baseline and to each other in their overlaps (pf_register_consistent); < 0: off
    double consistent = -1.0;
    // PF_TILE_WEIGHTS=tent|files:SUFFIX (panofuse_main --tile-weights): the per-pixel tile weights
    // of this call; without it SetTileWeights'
    pfw::Spec weights;
    // PF_DISPARITY_WEIGHTS=tent|files:SUFFIX|range:LO:HI (panofuse_main --disparity-weights): the
    // per-pixel weights of this call's disparity tiles; without it SetDisparityWeights'
    pfdw::Spec disp_weights;
};

// A finite LAMBDA >= 0, the whole string.
bool parse_lambda(const char* s, double& v)
{
    char* end = nullptr;
    v = std::strtod(s ? s : "", &end);
    return s && *s && end && *end == '\0' && v >= 0.0 && v < HUGE_VAL;
}

bool read_merge_switches(MergeSwitches& s)
{
    const auto env_on = [](const char* name) {
        const char* v = std::getenv(name);
        return v && std::strcmp(v, "1") == 0;
    };
    if (const char* fu = std::getenv("PF_FUSION")) {
        if (std::strcmp(fu, "smoothing") == 0) s.fusion = MergeSwitches::SMOOTHING;
        else if (std::strcmp(fu, "stitch") == 0) s.fusion = MergeSwitches::STITCH;
        else if (*fu && std::strcmp(fu, "laplacian") != 0) {
            std::cout << "[MergeDepthMaps] bad PF_FUSION " << fu
                      << " (want laplacian, smoothing or stitch)" << std::endl;
            return false;
        }
    }
    s.rule = tile_rule();
    if (const char* tv = std::getenv("PF_TILE_VALID")) {
        std::string err;
        if (!pfv::parse_range(tv, s.rule.lo, s.rule.hi, err)) {
            std::cout << "[MergeDepthMaps] PF_TILE_VALID: " << err << std::endl;
            return false;
        }
        s.rule.on = true;
    }
    s.loss = reg_loss();
    if (const char* rl = std::getenv("PF_REG_LOSS")) {
        if (!parse_reg_loss(rl, s.loss)) {
            std::cout << "[MergeDepthMaps] bad PF_REG_LOSS " << rl
                      << " (want huber:A or softl1:A, A > 0)" << std::endl;
            return false;
        }
    }
    s.tile_depth = tile_depth();
    if (const char* td = std::getenv("PF_TILE_DEPTH")) {
        s.tile_depth = pf::parse_tile_depth(td);
        if (s.tile_depth < 0) {
            std::cout << "[MergeDepthMaps] bad PF_TILE_DEPTH " << td << " (want planar or ray)"
                      << std::endl;
            return false;
        }
    }
    if (const char* rc = std::getenv("PF_REG_CONSISTENT")) {
        if (!parse_lambda(rc, s.consistent)) {
            std::cout << "[MergeDepthMaps] bad PF_REG_CONSISTENT " << rc
                      << " (want a finite LAMBDA >= 0)" << std::endl;
            return false;
        }
    }
    s.weights = tile_weights();
    if (const char* tw = std::getenv("PF_TILE_WEIGHTS")) {
        std::string err;
        if (!pfw::parse_spec(tw, s.weights, err)) {
            std::cout << "[MergeDepthMaps] PF_TILE_WEIGHTS: " << err << std::endl;
            return false;
        }
    }
    s.disp_weights = disparity_weights();
    if (const char* dw = std::getenv("PF_DISPARITY_WEIGHTS")) {
        std::string err;
        if (!pfdw::parse_spec(dw, s.disp_weights, err)) {
            std::cout << "[MergeDepthMaps] PF_DISPARITY_WEIGHTS: " << err << std::endl;
            return false;
        }
    }
    s.save_stitch = env_on("PF_SAVE_STITCH");
    s.check_laplacian = env_on("PF_CHECK_LAPLACIAN");
    s.global_align = env_on("PF_GLOBAL_ALIGN");
    if (s.check_laplacian && s.fusion != MergeSwitches::LAPLACIAN) {
        std::cout << "[MergeDepthMaps] PF_CHECK_LAPLACIAN needs PF_FUSION=laplacian: only the "
                     "fusion has Laplacian targets" << std::endl;
        return false;
    }
    return true;
}

int elapsed_ms(std::chrono::steady_clock::time_point t0)
{
    return (int)std::chrono::duration_cast<std::chrono::milliseconds>(
               std::chrono::steady_clock::now() - t0)
        .count();
}

// MergeDepthMaps stores MIN2(range, D2R(359.9)) (Depth.cpp:783-784: a float against a double,
// the double result rounded back to float).
float cap_range(float r)
{
    const double cap = PF_D2R(359.9);
    return (float)((double)r < cap ? (double)r : cap);
}

// The baseline and the tiles from their files, the tiles with their windows and ranges
// (Depth.cpp:773-787); the tiles decode in parallel host threads (zlib inflate is the host cost).
bool load_maps(std::string& emap_fn, std::vector<std::string>& pmap_fns, std::vector<Vec4f>& fovs,
               std::vector<Vec4f>& ranges, EquirectangularMap& emap,
               std::vector<PerspectiveMap>& pmaps)
{
    if (!emap.Load(emap_fn)) return false;
    if (fovs.size() < pmap_fns.size() || ranges.size() < pmap_fns.size()) {
        std::cout << "[MergeDepthMaps] fewer FOVs/ranges than maps" << std::endl;
        return false;
    }
    pmaps.resize(pmap_fns.size());
    std::vector<std::future<bool>> loads;
    for (size_t i = 0; i < pmap_fns.size(); i++)
        loads.push_back(
            std::async(std::launch::async, [&, i] { return pmaps[i].Load(pmap_fns[i]); }));
    bool ok = true;
    for (auto& f : loads) ok = f.get() && ok;
    if (!ok) return false;
    for (size_t i = 0; i < pmap_fns.size(); i++) {
        PerspectiveMap& p = pmaps[i];
        p.SetWindow(fovs[i][0], fovs[i][1], fovs[i][2], fovs[i][3]);
        p.ranges = Vec4f(cap_range(ranges[i][0]), cap_range(ranges[i][1]), ranges[i][2],
                         ranges[i][3]);
    }
    return true;
}

// What the GPU steps work on: the baseline, the packed tiles, the per-tile cubics the fusion
// applies (null for disparity tiles, which the registration has transformed already) and the
// u16 result, all on the device.
struct Job {
    pf_ctx* c;
    const EquirectangularMap& emap;
    const float* d_emap;
    float* d_tiles;  // the disparity registration transforms them in place
    const float* d_coeffs;
    uint16_t* d_out;
    int w, h;
    Vec2f& zr;
};

// Registration (Depth.cpp:789-808): every tile alone; depth tiles: cubic, the transform fused
// into the fusion; disparity tiles: y = 1/(a x + b) + d, D2DTransform on the uploaded copy.
bool register_tiles(const Job& j, float* d_coeffs, bool disparity_tiles, int ntiles,
                    const RegLossRule& loss, bool planar)
{
    const EquirectangularMap& e = j.emap;
    // planar-depth tiles: the cubic is applied to the uploaded tiles too (with the ray factor),
    // and the fusion then runs without coefficients
    const int apply = planar ? 1 : 0;
    if (loss.kind != PF_LOSS_NONE) {  // the same calls with the solver summary, one line per tile
        static const char* const kTerm[] = {"no convergence", "function tolerance",
                                            "parameter tolerance", "gradient tolerance",
                                            "minimum trust-region radius", "failure"};
        DevMem ds(sizeof(double) * 6 * ntiles);
        std::vector<double> sm((size_t)6 * ntiles);
        if (!ds.ok ||
            !call_sync(j.c,
                       disparity_tiles
                           ? pf_register_disparity(j.c, j.d_emap, e.width, e.height, e.channels,
                                                   j.d_tiles, 1, j.zr[0], j.zr[1], 1, d_coeffs,
                                                   nullptr, ds.as<double>())
                           : pf_register_ex(j.c, j.d_emap, e.width, e.height, e.channels,
                                            j.d_tiles, 1, j.zr[0], j.zr[1], 3, apply, d_coeffs,
                                            nullptr, ds.as<double>()),
                       disparity_tiles ? "pf_register_disparity" : "pf_register_ex") ||
            !download(sm.data(), ds, sm.size()))
            return false;
        for (int p = 0; p < ntiles; p++) {
            const double* s = &sm[(size_t)6 * p];
            const int term = s[3] >= 0 && s[3] <= 5 ? (int)s[3] : 5;
            std::cout << "[robust] tile " << p << ": " << (long long)(s[4] - s[5]) << " of "
                      << (long long)s[4] << " samples beyond a=" << loss.a << ", cost " << s[0]
                      << " -> " << s[1] << ", " << (int)s[2] << " iterations, " << kTerm[term]
                      << std::endl;
        }
        return true;
    }
    return call_sync(j.c,
                     disparity_tiles
                         ? pf_register_disparity(j.c, j.d_emap, e.width, e.height, e.channels,
                                                 j.d_tiles, 1, j.zr[0], j.zr[1], 1, d_coeffs,
                                                 nullptr, nullptr)
                         : pf_register(j.c, j.d_emap, e.width, e.height, e.channels, j.d_tiles, 1,
                                       j.zr[0], j.zr[1], 3, apply, d_coeffs, nullptr),
                     disparity_tiles ? "pf_register_disparity" : "pf_register");
}

// sqrt(sum sum d^2 / sum count) over the pairs of pf_overlap_stats under coeffs.
bool overlap_rms(const Job& j, const float* d_coeffs, int npairs, double& rms)
{
    DevMem ds(sizeof(double) * 5 * (size_t)npairs);
    std::vector<double> st((size_t)5 * npairs);
    if (!ds.ok ||
        !call_sync(j.c, pf_overlap_stats(j.c, j.d_tiles, d_coeffs, 1, j.zr[0], j.zr[1],
                                         ds.as<double>()),
                   "pf_overlap_stats") ||
        !download(st.data(), ds, st.size()))
        return false;
    double n = 0.0, dd = 0.0;
    for (int i = 0; i < npairs; i++) {
        n = n + st[(size_t)5 * i];
        dd = dd + st[(size_t)5 * i + 2];
    }
    rms = n > 0.0 ? std::sqrt(dd / n) : 0.0;
    return true;
}

// PF_REG_CONSISTENT: the tiles registered together (pf_register_consistent) instead of one by one,
// and "[consistent] lambda <L>: <P> pairs, <S> pair samples, overlap rms <before> -> <after>",
// before under the independent coefficients of pf_register, after under the consistent ones.
bool register_consistent(const Job& j, float* d_coeffs, int ntiles, double lambda)
{
    const EquirectangularMap& e = j.emap;
    int npairs = 0;
    long long nsamples = 0;
    if (!pf_ok(j.c, pf_overlap_pairs(j.c, j.zr[0], j.zr[1], &npairs, &nsamples), "pf_overlap_pairs"))
        return false;
    DevMem dind(sizeof(float) * 4 * ntiles), dsum(sizeof(double) * 4);
    double before = 0.0, after = 0.0, sm[4];
    if (!dind.ok || !dsum.ok ||
        !pf_ok(j.c, pf_register(j.c, j.d_emap, e.width, e.height, e.channels, j.d_tiles, 1, j.zr[0],
                                j.zr[1], 3, 0, dind.as<float>(), nullptr),
               "pf_register") ||
        (npairs > 0 && !overlap_rms(j, dind.as<float>(), npairs, before)) ||
        !call_sync(j.c, pf_register_consistent(j.c, j.d_emap, e.width, e.height, e.channels,
                                               j.d_tiles, 1, j.zr[0], j.zr[1], lambda, 0, d_coeffs,
                                               nullptr, dsum.as<double>()),
                   "pf_register_consistent") ||
        !download(sm, dsum, 4))
        return false;
    if (sm[3] != 0.0) {
        std::cout << "[MergeDepthMaps] pf_register_consistent: the joint system is singular"
                  << std::endl;
        return false;
    }
    if (npairs > 0 && !overlap_rms(j, d_coeffs, npairs, after)) return false;
    char line[192];
    std::snprintf(line, sizeof(line),
                  "[consistent] lambda %g: %d pairs, %lld pair samples, overlap rms %.6g -> %.6g",
                  lambda, npairs, nsamples, before, after);
    std::cout << line << std::endl;
    return true;
}

// What the weighted forms cannot be combined with (pf_register_weighted / pf_fuse_weighted have no
// form for it), or nullptr.
const char* weights_conflict(const MergeSwitches& s, bool disparity_tiles)
{
    if (disparity_tiles) return "disparity tiles";
    if (s.rule.on) return "the tile validity rule (PF_TILE_VALID / SetTileValidity)";
    if (s.loss.kind != PF_LOSS_NONE) return "a registration loss (PF_REG_LOSS / SetRegistrationLoss)";
    if (s.tile_depth != PF_TILE_DEPTH_RAY) return "planar-depth tiles (PF_TILE_DEPTH / SetTileDepth)";
    if (s.consistent >= 0.0) return "PF_REG_CONSISTENT";
    if (s.global_align) return "PF_GLOBAL_ALIGN";
    if (s.fusion == MergeSwitches::SMOOTHING) return "PF_FUSION=smoothing";
    if (s.fusion == MergeSwitches::STITCH) return "PF_FUSION=stitch";
    if (s.check_laplacian) return "PF_CHECK_LAPLACIAN";
    return nullptr;
}

// The weight set of this call on the device, in the packed tiles' layout (one channel): the tent,
// or channel 0 of every tile file's weight map F + SUFFIX, which must have the tile's size.
DevMem weights_on_device(pf_ctx* c, const pfw::Spec& spec, const std::vector<std::string>& pmap_fns,
                         const std::vector<PerspectiveMap>& pmaps)
{
    DevMem none(0);
    none.ok = false;
    size_t total = 0;
    for (const PerspectiveMap& p : pmaps) total += (size_t)p.width * p.height;
    if (spec.mode == pfw::TENT) {
        DevMem dw(sizeof(float) * total);
        if (!dw.ok || !pf_ok(c, pf_tile_tent_weights(c, dw.as<float>()), "pf_tile_tent_weights"))
            return none;
        return dw;
    }
    std::vector<float> packed(total);
    size_t off = 0;
    for (size_t i = 0; i < pmaps.size(); i++) {
        std::string fn = pfw::weight_file(pmap_fns[i], spec), err;
        // a PFM is read raw (its floats as stored, rows in file order: the map loaders would scale
        // them as depth in metres), anything else as a tile is: a PNG's samples in 0-1
        const bool pfm = fn.size() >= 3 && fn.compare(fn.size() - 3, 3, "pfm") == 0;
        PerspectiveMap img;
        int w = 0, h = 0, ch = 0;
        float* raw = pfm ? pfio::load_pfm(fn, &w, &h, &ch, err) : nullptr;
        if (pfm ? !raw : !img.Load(fn)) {
            std::cout << "[MergeDepthMaps] cannot load the weight map " << fn
                      << (err.empty() ? "" : ": ") << err << std::endl;
            return none;
        }
        if (!pfm) w = img.width, h = img.height, ch = img.channels;
        const float* px = pfm ? raw : img.data;
        const bool fits = pfw::size_matches(fn, w, h, pmaps[i].width, pmaps[i].height, err);
        if (fits) {
            const size_t n = (size_t)w * h;
            for (size_t k = 0; k < n; k++) packed[off + k] = px[k * ch];
            off += n;
        } else {
            std::cout << "[MergeDepthMaps] " << err << std::endl;
        }
        std::free(raw);
        if (!fits) return none;
    }
    return DevMem(packed.data(), packed.size());
}

// The weighted registration (pf_register_weighted, the tiles untouched) and one "[weights] tile
// <i>: <n> of <N> samples used, sum w <s>" line per tile.
bool register_weighted(const Job& j, float* d_coeffs, const float* d_weights, int ntiles)
{
    const EquirectangularMap& e = j.emap;
    DevMem ds(sizeof(double) * 2 * ntiles), dn(sizeof(long long) * 2 * ntiles);
    std::vector<double> sm((size_t)2 * ntiles);
    std::vector<long long> total((size_t)2 * ntiles);
    if (!ds.ok || !dn.ok ||
        !pf_ok(j.c, pf_tile_valid_counts(j.c, j.d_tiles, j.d_emap, e.width, e.height, e.channels, 1,
                                         j.zr[0], j.zr[1], dn.as<long long>()),
               "pf_tile_valid_counts") ||
        !call_sync(j.c, pf_register_weighted(j.c, j.d_emap, e.width, e.height, e.channels,
                                             j.d_tiles, d_weights, 1, 1, j.zr[0], j.zr[1], 0,
                                             d_coeffs, nullptr, ds.as<double>()),
                   "pf_register_weighted") ||
        !download(sm.data(), ds, sm.size()) || !download(total.data(), dn, total.size()))
        return false;
    for (int p = 0; p < ntiles; p++)
        std::cout << pfw::weights_line(p, sm[(size_t)2 * p], total[(size_t)2 * p],
                                       sm[(size_t)2 * p + 1])
                  << std::endl;
    return true;
}

// What stands beside PF_DISPARITY_WEIGHTS / SetDisparityWeights in this call (pfdw::clash names
// the first it has no form for).
pfdw::Others disp_weights_others(const MergeSwitches& s, bool disparity_tiles)
{
    pfdw::Others o;
    o.disparity_tiles = disparity_tiles;
    o.tile_valid = s.rule.on;
    o.reg_loss = s.loss.kind != PF_LOSS_NONE;
    o.consistent = s.consistent >= 0.0;
    o.global_align = s.global_align;
    o.check_laplacian = s.check_laplacian;
    o.tile_weights = s.weights.mode != pfw::OFF;
    o.smoothing = s.fusion == MergeSwitches::SMOOTHING;
    o.stitch = s.fusion == MergeSwitches::STITCH;
    return o;
}

// The weighted disparity merge (pf_merge_disparity_weighted: the fit with apply on the library's
// copy, then the weighted fusion of that copy), then the fit once more for its summary: one
// "[weights] tile <i>: <n> of <N> samples used, sum w <s>" line per tile.  The merge has no
// summary of its own, so the lines cost a second fit; with apply_after it transforms the uploaded
// tiles as well, which is what PF_SAVE_STITCH stitches.
bool merge_disparity_weighted(const Job& j, float* d_coeffs, const float* d_weights, int ntiles,
                              bool apply_after)
{
    const EquirectangularMap& e = j.emap;
    DevMem ds(sizeof(double) * 6 * ntiles), dn(sizeof(long long) * 2 * ntiles);
    std::vector<double> sm((size_t)6 * ntiles);
    std::vector<long long> total((size_t)2 * ntiles);
    if (!ds.ok || !dn.ok ||
        !pf_ok(j.c, pf_tile_valid_counts(j.c, j.d_tiles, j.d_emap, e.width, e.height, e.channels, 1,
                                         j.zr[0], j.zr[1], dn.as<long long>()),
               "pf_tile_valid_counts") ||
        !pf_ok(j.c, pf_merge_disparity_weighted(j.c, j.d_emap, e.width, e.height, e.channels,
                                                j.d_tiles, d_weights, 1, 1, j.w, j.zr[0], j.zr[1],
                                                d_coeffs, j.d_out),
               "pf_merge_disparity_weighted") ||
        !call_sync(j.c, pf_register_disparity_weighted(j.c, j.d_emap, e.width, e.height,
                                                       e.channels, j.d_tiles, d_weights, 1, 1,
                                                       j.zr[0], j.zr[1], apply_after ? 1 : 0,
                                                       nullptr, nullptr, ds.as<double>()),
                   "pf_register_disparity_weighted") ||
        !download(sm.data(), ds, sm.size()) || !download(total.data(), dn, total.size()))
        return false;
    for (int p = 0; p < ntiles; p++)
        std::cout << pfw::weights_line(p, sm[(size_t)6 * p + 4], total[(size_t)2 * p],
                                       sm[(size_t)6 * p + 5])
                  << std::endl;
    return true;
}

// The fusion (Depth.cpp:904-913), or the smoothing (:919-922) / the stitch (:851) on the
// registered tiles.
bool fuse(const Job& j, const MergeSwitches& s)
{
    const EquirectangularMap& e = j.emap;
    switch (s.fusion) {
    case MergeSwitches::SMOOTHING:
        return call_sync(j.c, pf_solve_smoothing(j.c, j.d_tiles, j.d_coeffs, 1, j.w, j.h, j.zr[0],
                                                 j.zr[1], j.d_out),
                         "pf_solve_smoothing");
    case MergeSwitches::STITCH:
        return call_sync(j.c, pf_stitch(j.c, j.d_tiles, j.d_coeffs, 1, j.w, j.h, j.d_out),
                         "pf_stitch");
    default:
        return call_sync(j.c, pf_fuse(j.c, j.d_emap, e.width, e.height, e.channels, j.d_tiles,
                                      j.d_coeffs, 1, j.w, j.h, j.zr[0], j.zr[1], j.d_out),
                         "pf_fuse");
    }
}

// Under the validity rule: one "[mask] tile <i>: ..." line per tile that has invalid pixels, from
// pf_tile_valid_counts under the rule and, for the totals, without it.
bool print_mask_lines(const Job& j, int ntiles, const TileRule& rule)
{
    const EquirectangularMap& e = j.emap;
    const size_t n = (size_t)ntiles * 2;
    DevMem dv(sizeof(long long) * n), dt(sizeof(long long) * n);
    std::vector<long long> valid(n), total(n);
    const auto counts = [&](DevMem& d) {
        return pf_tile_valid_counts(j.c, j.d_tiles, j.d_emap, e.width, e.height, e.channels, 1,
                                    j.zr[0], j.zr[1], d.as<long long>());
    };
    if (!dv.ok || !dt.ok || !pf_ok(j.c, counts(dv), "pf_tile_valid_counts")) return false;
    pf_set_tile_validity(j.c, PF_VALID_ALL, 0.0f, 0.0f);
    const int rc = counts(dt);
    apply_rule(j.c, rule);
    if (!call_sync(j.c, rc, "pf_tile_valid_counts") || !download(valid.data(), dv, n) ||
        !download(total.data(), dt, n))
        return false;
    std::vector<std::string> lines;
    if (!pfv::mask_lines(valid.data(), total.data(), ntiles, lines)) {
        std::cout << "[MergeDepthMaps] inconsistent validity counts" << std::endl;
        return false;
    }
    for (const std::string& ln : lines) std::cout << ln << std::endl;
    return true;
}

// "[tile-depth] planar: ray factor up to <max kf> over <n> tiles", from the layout's tables.
bool print_tile_depth_line(pf_ctx* c, const std::vector<PerspectiveMap>& pmaps)
{
    float top = 1.0f;
    for (size_t p = 0; p < pmaps.size(); p++) {
        std::vector<double> cu((size_t)pmaps[p].width), rv((size_t)pmaps[p].height);
        if (!pf_ok(c, pf_tile_ray_tables(c, (int)p, cu.data(), rv.data()), "pf_tile_ray_tables"))
            return false;
        double mu = 0.0, mv = 0.0;
        for (double v : cu) mu = v > mu ? v : mu;
        for (double v : rv) mv = v > mv ? v : mv;
        const float k = pf::ray_factor(mu, mv);
        top = k > top ? k : top;
    }
    char line[128];
    std::snprintf(line, sizeof(line), "[tile-depth] planar: ray factor up to %.3f over %zu tiles",
                  (double)top, pmaps.size());
    std::cout << line << std::endl;
    return true;
}

// Depth.cpp:1738-1758: the last level's number, in the reference's words.
bool print_laplacian_check(const Job& j)
{
    const EquirectangularMap& e = j.emap;
    int nlevels = 0;
    DevMem derr(sizeof(float) * 4);
    float err[4] = {};
    if (!derr.ok ||
        !pf_ok(j.c, pf_level_info(j.w, j.h, j.zr[0], j.zr[1], 0, nullptr, nullptr, nullptr, nullptr,
                                  nullptr, &nlevels),
               "pf_level_info") ||
        nlevels < 1 || nlevels > 4 ||
        !call_sync(j.c, pf_fuse_check(j.c, j.d_emap, e.width, e.height, e.channels, j.d_tiles,
                                      j.d_coeffs, j.w, j.h, j.zr[0], j.zr[1], derr.as<float>(),
                                      nullptr),
                   "pf_fuse_check") ||
        !download(err, derr, nlevels))
        return false;
    std::cout << std::endl << "[SolveDepthAll] check Laplacian err:" << err[nlevels - 1]
              << std::endl;
    return true;
}

// Depth.cpp:817-865: <out>.pmap.png, the direct stitch of the registered tiles.
bool save_stitch(const Job& j, const std::string& out_fn)
{
    const size_t no = (size_t)j.w * j.h;
    DevMem ds(no * 2);
    std::vector<unsigned short> st(no);
    return ds.ok &&
           call_sync(j.c, pf_stitch(j.c, j.d_tiles, j.d_coeffs, 1, j.w, j.h, ds.as<uint16_t>()),
                     "pf_stitch") &&
           download(st.data(), ds, no) &&
           Save16BitPNG(st.data(), j.w, j.h, (out_fn + ".pmap.png").c_str());
}

// A u16 map masked by the gt's invalid (0) / saturated pixels and the zenith band.
template <class ValueAt>
void save_masked(EquirectangularMap& gt, Vec2f& zr, int w, int h, ValueAt value_at,
                 const std::string& fn)
{
    const int h0 = (int)std::floor(h * zr[0] / PF_MYPI_D);
    const int h1 = (int)std::ceil(h * zr[1] / PF_MYPI_D);
    std::vector<unsigned short> o((size_t)w * h);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            unsigned short& d = o[(size_t)y * w + x];
            if (y < h0 || y > h1) {
                d = 0;
                continue;
            }
            const int X = (int)((float)x * (float)gt.width / (float)w);
            const int Y = (int)((float)y * (float)gt.height / (float)h);
            const float g = gt.ValueAtXY(X, Y);
            d = g == 0 ? 0 : ((double)g >= 1 - 1e-4 ? 65535 : value_at(x, y));
        }
    Save16BitPNG(o.data(), w, h, fn.c_str());
}

// Depth.cpp:920-1037: the baseline's and the result's metrics against the gt, printed, and the
// two masked maps <out>.res.png / <out>.giv.png (the first on a host thread beside the second).
void score_and_mask(EquirectangularMap& gt, EquirectangularMap& emap,
                    std::vector<unsigned short>& data, int w, int h, Vec2f& zr,
                    const std::string& out_fn, Metrics* metrics)
{
    const int align_way = 1;
    const bool cap_depth = true;
    Metrics local;
    Metrics& M = metrics ? *metrics : local;
    ErrorEmap(gt, emap, M.mse_given, M.mae_given, M.mre_given, M.mselog_given, M.delta1_given,
              M.delta2_given, M.delta3_given, align_way, cap_depth);
    ErrorData(gt, data.data(), w, h, M.mse_result, M.mae_result, M.mre_result, M.mselog_result,
              M.delta1_result, M.delta2_result, M.delta3_result, align_way, cap_depth);
    M.Print();
    auto res = std::async(std::launch::async, [&] {
        save_masked(gt, zr, w, h, [&](int x, int y) { return data[(size_t)y * w + x]; },
                    out_fn + ".res.png");
    });
    save_masked(gt, zr, emap.width, emap.height,
                [&](int x, int y) { return (unsigned short)(emap.ValueAtXY(x, y) * 65535.0f); },
                out_fn + ".giv.png");
    res.get();
}

// The body of MergeDepthMaps for depth tiles, or with disparity_tiles for tiles that hold
// relative inverse depth (MergeDisparityMaps): only the registration differs.
bool merge_maps(std::string& emap_fn, std::vector<std::string>& pmap_fns, std::string& out_fn,
                std::vector<Vec4f>& fovs, std::vector<Vec4f>& ranges, int out_width, Vec2f& zr,
                std::string* gt_fn, Metrics* metrics, int* time_Reg, int* time_Laplacian,
                bool disparity_tiles)
{
    const auto t_begin = std::chrono::steady_clock::now();
    MergeSwitches sw;
    if (!read_merge_switches(sw)) return false;
    // the disparity tiles' weights stand alone too: refused before any file is read
    const bool disp_weighted = sw.disp_weights.mode != pfdw::OFF;
    if (disp_weighted) {
        if (const char* what = pfdw::clash(disp_weights_others(sw, disparity_tiles), false)) {
            std::cout << "[MergeDepthMaps] " << pfdw::clash_message(what, false) << std::endl;
            return false;
        }
    }
    // the weighted forms stand alone: refused before any file is read
    const bool weighted = sw.weights.mode != pfw::OFF;
    if (weighted) {
        if (const char* what = weights_conflict(sw, disparity_tiles)) {
            std::cout << "[MergeDepthMaps] tile weights (PF_TILE_WEIGHTS / SetTileWeights) have no "
                         "form for "
                      << what << ": switch one of the two off" << std::endl;
            return false;
        }
    }
    // the entry points that cannot honour the validity rule: refused before any file is read
    if (sw.rule.on && (disparity_tiles || sw.fusion == MergeSwitches::SMOOTHING)) {
        std::cout << "[MergeDepthMaps] "
                  << (disparity_tiles ? "pf_register_disparity" : "pf_solve_smoothing")
                  << " does not honour the tile validity rule (pf_set_tile_validity): unset "
                     "PF_TILE_VALID / SetTileValidity(false, 0, 0), or use depth tiles with "
                     "PF_FUSION=laplacian or stitch"
                  << std::endl;
        return false;
    }
    // the global fit has no robust form: refused with the library's message before any file is read
    if (sw.loss.kind != PF_LOSS_NONE && sw.global_align) {
        if (pf_ctx* c = facade_ctx()) {
            apply_loss(c, sw.loss);
            pf_ok(c, pf_register_global(c, nullptr, 0, 0, 0, nullptr, 1, 0, 0, 0.0f, 0.0f, 0,
                                        nullptr, nullptr, nullptr),
                  "pf_register_global");
            apply_loss(c, reg_loss());
        }
        return false;
    }
    // the consistent registration: depth tiles only, no global fit after it; under a mode it has no
    // form for, the library's message -- all before any file is read
    if (sw.consistent >= 0.0) {
        if (disparity_tiles || sw.global_align) {
            std::cout << "[MergeDepthMaps] PF_REG_CONSISTENT registers depth tiles by a linear "
                         "solve: not with "
                      << (disparity_tiles ? "disparity tiles" : "PF_GLOBAL_ALIGN") << std::endl;
            return false;
        }
        if (sw.rule.on || sw.loss.kind != PF_LOSS_NONE || sw.tile_depth != PF_TILE_DEPTH_RAY) {
            if (pf_ctx* c = facade_ctx()) {
                apply_rule(c, sw.rule);
                apply_loss(c, sw.loss);
                pf_set_tile_depth(c, sw.tile_depth);
                pf_ok(c, pf_register_consistent(c, nullptr, 0, 0, 0, nullptr, 1, 0.0f, 0.0f,
                                                sw.consistent, 0, nullptr, nullptr, nullptr),
                      "pf_register_consistent");
                apply_rule(c, tile_rule());
                apply_loss(c, reg_loss());
                pf_set_tile_depth(c, tile_depth());
            }
            return false;
        }
    }
    EquirectangularMap emap, gt;
    std::vector<PerspectiveMap> pmaps;
    // the ground truth decodes on a host thread while the tiles load and the GPU fuses
    std::future<bool> gt_loaded;
    if (gt_fn) gt_loaded = std::async(std::launch::async, [&] { return gt.Load(*gt_fn); });
    struct Join {  // never leave with the loader still writing into `gt`
        std::future<bool>& f;
        ~Join()
        {
            if (f.valid()) f.wait();
        }
    } join{gt_loaded};
    if (!load_maps(emap_fn, pmap_fns, fovs, ranges, emap, pmaps)) return false;
    const int out_height = out_width / 2;
    const size_t no = (size_t)out_width * out_height;

    pf_ctx* c = facade_ctx();
    if (!c) return false;
    // this call's rule (PF_TILE_VALID over SetTileValidity's); the stored one comes back at exit
    struct RuleScope {
        pf_ctx* c;
        ~RuleScope()
        {
            apply_rule(c, tile_rule());
            apply_loss(c, reg_loss());
            pf_set_tile_depth(c, tile_depth());
        }
    } rule_scope{c};
    if (!pf_ok(c, apply_rule(c, sw.rule), "pf_set_tile_validity")) return false;
    if (!pf_ok(c, apply_loss(c, sw.loss), "pf_set_register_loss")) return false;
    if (!pf_ok(c, pf_set_tile_depth(c, sw.tile_depth), "pf_set_tile_depth")) return false;
    const bool planar = sw.tile_depth == PF_TILE_DEPTH_PLANAR;
    DevMem dt = tiles_on_device(c, pmaps);
    if (!dt.ok) return false;
    DevMem de = on_device(emap), dc(sizeof(float) * 4 * pmaps.size()), dout(no * 2);
    if (!de.ok || !dc.ok || !dout.ok) return false;
    const Job j{c, emap, de.as<float>(), dt.as<float>(),
                disparity_tiles || planar ? nullptr : dc.as<float>(), dout.as<uint16_t>(),
                out_width, out_height, zr};
    if (planar && !print_tile_depth_line(c, pmaps)) return false;

    if (sw.rule.on && !print_mask_lines(j, (int)pmaps.size(), sw.rule)) return false;
    DevMem dw = weighted ? weights_on_device(c, sw.weights, pmap_fns, pmaps) : DevMem(0);
    if (!dw.ok) return false;
    if (disp_weighted) {  // nothing else is on (pfdw::clash): the weighted disparity merge
        size_t total = 0;
        for (const PerspectiveMap& p : pmaps) total += (size_t)p.width * p.height;
        DevMem dd = sw.disp_weights.mode == pfdw::RANGE
                        ? DevMem(sizeof(float) * total)
                        : weights_on_device(c, pfdw::as_tile_spec(sw.disp_weights), pmap_fns, pmaps);
        if (!dd.ok) return false;
        if (sw.disp_weights.mode == pfdw::RANGE &&
            !pf_ok(c, pf_tile_range_weights(c, j.d_tiles, 1, sw.disp_weights.lo,
                                            sw.disp_weights.hi, dd.as<float>()),
                   "pf_tile_range_weights"))
            return false;
        const auto t0 = std::chrono::steady_clock::now();
        if (!merge_disparity_weighted(j, dc.as<float>(), dd.as<float>(), (int)pmaps.size(),
                                      sw.save_stitch))
            return false;
        if (time_Reg) *time_Reg = 0;  // one call fits and fuses
        if (time_Laplacian) *time_Laplacian = elapsed_ms(t0);
    } else {
        auto t = std::chrono::steady_clock::now();
        // with weights nothing else is on (weights_conflict): the weighted pair of calls
        if (weighted ? !register_weighted(j, dc.as<float>(), dw.as<float>(), (int)pmaps.size())
            : sw.consistent >= 0.0
                ? !register_consistent(j, dc.as<float>(), (int)pmaps.size(), sw.consistent)
                : !register_tiles(j, dc.as<float>(), disparity_tiles, (int)pmaps.size(), sw.loss,
                                  planar))
            return false;
        // the transformed planar tiles carry NaN at their invalid pixels: what follows reads them
        // under (-inf, +inf), not under the caller's lo / hi (a value clamped to exactly 0 is valid)
        if (planar && sw.rule.on &&
            !pf_ok(c, apply_rule(c, TileRule{true, -INFINITY, INFINITY}), "pf_set_tile_validity"))
            return false;
        if (time_Reg) *time_Reg = elapsed_ms(t);
        t = std::chrono::steady_clock::now();
        if (weighted ? !call_sync(c, pf_fuse_weighted(c, j.d_emap, emap.width, emap.height,
                                                      emap.channels, j.d_tiles, dw.as<float>(), 1,
                                                      j.d_coeffs, 1, j.w, j.h, zr[0], zr[1],
                                                      j.d_out),
                                  "pf_fuse_weighted")
                     : !fuse(j, sw))
            return false;
        if (time_Laplacian) *time_Laplacian = elapsed_ms(t);
    }
    if (sw.check_laplacian && !print_laplacian_check(j)) return false;
    if (sw.save_stitch && !save_stitch(j, out_fn)) return false;
    Vec4f g;
    if (sw.global_align &&
        !global_fit(c, j.d_emap, emap, j.d_out, out_width, out_height, zr, true, g))
        return false;

    std::vector<unsigned short> data(no);
    if (!download(data.data(), dout, no) ||
        !Save16BitPNG(data.data(), out_width, out_height, out_fn.c_str()))
        return false;
    std::cout << "...All done! @" << elapsed_ms(t_begin) << std::endl;
    if (gt_fn && gt_loaded.get())
        score_and_mask(gt, emap, data, out_width, out_height, zr, out_fn, metrics);
    return true;
}
}  // namespace

bool MergeDepthMaps(std::string& emap_fn, std::vector<std::string>& pmap_fns,
                    std::string& out_fn, std::vector<Vec4f>& fovs, std::vector<Vec4f>& ranges,
                    int out_width, Vec2f& zr, std::string* gt_fn, Metrics* metrics,
                    int* time_Reg, int* time_Laplacian)
{
    return merge_maps(emap_fn, pmap_fns, out_fn, fovs, ranges, out_width, zr, gt_fn, metrics,
                      time_Reg, time_Laplacian, false);
}

bool MergeDisparityMaps(std::string& emap_fn, std::vector<std::string>& pmap_fns,
                        std::string& out_fn, std::vector<Vec4f>& fovs,
                        std::vector<Vec4f>& ranges, int out_width, Vec2f& zr,
                        std::string* gt_fn, Metrics* metrics, int* time_Reg,
                        int* time_Laplacian)
{
    return merge_maps(emap_fn, pmap_fns, out_fn, fovs, ranges, out_width, zr, gt_fn, metrics,
                      time_Reg, time_Laplacian, true);
}

}  // namespace DepthNamespace
