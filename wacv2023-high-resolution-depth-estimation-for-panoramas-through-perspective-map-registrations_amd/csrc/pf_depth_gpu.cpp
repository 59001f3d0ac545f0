// pf_depth_gpu.cpp -- the entry points of the DepthNamespace facade (include/pf_depth.h) that
// are one libpanofuse call each: the solvers, the in-place transforms, MedianScaling,
// TransformResult, ErrorData / ErrorEmap, ErrorCompare and ErrorLaplacian.  Each one checks its
// arguments, puts its inputs on the device (pf_facade.hpp), makes the one pf_* call and hands the
// result back; the files around them are host code (pf_depth_maps.cpp).
#include "pf_facade.hpp"

#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>

namespace pff __attribute__((visibility("hidden"))) {

static std::mutex g_rule_mu;
static TileRule g_rule{false, 0.0f, 0.0f};

TileRule tile_rule()
{
    std::lock_guard<std::mutex> lk(g_rule_mu);
    return g_rule;
}

static RegLossRule g_loss{PF_LOSS_NONE, 0.0};

RegLossRule reg_loss()
{
    std::lock_guard<std::mutex> lk(g_rule_mu);
    return g_loss;
}

static int g_tile_depth = PF_TILE_DEPTH_RAY;

int tile_depth()
{
    std::lock_guard<std::mutex> lk(g_rule_mu);
    return g_tile_depth;
}

static pfw::Spec g_tile_weights;

pfw::Spec tile_weights()
{
    std::lock_guard<std::mutex> lk(g_rule_mu);
    return g_tile_weights;
}

static pfdw::Spec g_disp_weights;

pfdw::Spec disparity_weights()
{
    std::lock_guard<std::mutex> lk(g_rule_mu);
    return g_disp_weights;
}

static pf_ctx* device_ctx();

pf_ctx* facade_ctx()
{
    pf_ctx* c = device_ctx();
    if (c) {
        apply_rule(c, tile_rule());  // a checked rule (SetTileValidity): cannot fail
        apply_loss(c, reg_loss());   // a checked loss (SetRegistrationLoss): neither
        pf_set_tile_depth(c, tile_depth());  // a checked kind (SetTileDepth): neither
    }
    return c;
}

static pf_ctx* device_ctx()
{
    static std::mutex mu;
    static std::map<int, pf_ctx*> ctxs;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    std::lock_guard<std::mutex> lk(mu);
    auto it = ctxs.find(dev);
    if (it != ctxs.end()) return it->second;
    pf_ctx* c = nullptr;
    if (pf_create(dev, &c) != PF_OK) {
        std::cout << "[panofuse] pf_create(" << dev << ") failed: no usable HIP device" << std::endl;
        return nullptr;
    }
    // ErrorData / ErrorEmap summation order: the facade mirrors Depth.cpp, so by default it sums
    // in the reference's row-major float order (the means the reference prints, bit for bit;
    // ~7.4 ms per 64-panorama call, well under a millisecond more at the facade's batch 1).
    // PF_METRICS_ORDER=tree (panofuse_main --metrics-order tree) opts into the fp64 tree.
    const char* mo = std::getenv("PF_METRICS_ORDER");
    pf_set_metrics_order(c, mo && std::strcmp(mo, "tree") == 0 ? PF_METRICS_TREE
                                                                : PF_METRICS_SEQUENTIAL);
    ctxs[dev] = c;
    return c;
}

DevMem tiles_on_device(pf_ctx* c, const std::vector<PerspectiveMap*>& pm)
{
    DevMem none(0);
    none.ok = false;
    std::vector<pf_window> fov(pm.size()), rng(pm.size());
    std::vector<int> tw(pm.size()), th(pm.size());
    size_t total = 0;
    for (size_t i = 0; i < pm.size(); ++i) {
        const PerspectiveMap& p = *pm[i];
        if (!p.data || !p.window_set) {
            std::cout << "[panofuse] perspective map " << i << " has no data or no window"
                      << std::endl;
            return none;
        }
        fov[i] = pf_window{p.azimuth_left, p.azimuth_right, p.zenith_top, p.zenith_down};
        rng[i] = to_window(p.ranges);
        tw[i] = p.width;
        th[i] = p.height;
        total += (size_t)p.width * p.height;
    }
    std::vector<float> packed(total);
    size_t off = 0;
    for (const PerspectiveMap* p : pm) {
        const size_t n = (size_t)p->width * p->height;
        for (size_t k = 0; k < n; ++k) packed[off + k] = p->data[k * p->channels];
        off += n;
    }
    if (!pf_ok(c, pf_set_tiles(c, fov.data(), rng.data(), (int)pm.size(), tw.data(), th.data(), 1,
                               0),
               "pf_set_tiles"))
        return none;
    return DevMem(packed.data(), packed.size());
}

DevMem tiles_on_device(pf_ctx* c, std::vector<PerspectiveMap>& pmaps)
{
    std::vector<PerspectiveMap*> pm;
    for (auto& p : pmaps) pm.push_back(&p);
    return tiles_on_device(c, pm);
}

std::vector<PerspectiveMap*> active_maps(std::vector<PerspectiveMap>& pmaps,
                                         const std::vector<bool>& actives)
{
    std::vector<PerspectiveMap*> pm;
    for (size_t i = 0; i < actives.size() && i < pmaps.size(); ++i)
        if (actives[i]) pm.push_back(&pmaps[i]);
    return pm;
}

bool global_fit(pf_ctx* c, const float* d_emap, const EquirectangularMap& emap, uint16_t* d_data,
                int w, int h, Vec2f& zr, bool apply, Vec4f& abcd)
{
    DevMem dc(4 * sizeof(float)), ds(4 * sizeof(double));
    if (!dc.ok || !ds.ok) return false;
    if (!call_sync(c, pf_register_global(c, d_emap, emap.width, emap.height, emap.channels, d_data,
                                         1, w, h, zr[0], zr[1], apply ? 1 : 0, dc.as<float>(),
                                         nullptr, ds.as<double>()),
                   "pf_register_global"))
        return false;
    float k[4];
    double sm[4];
    if (!download(k, dc, 4) || !download(sm, ds, 4)) return false;
    abcd = to_vec4(k);
    // Depth.cpp:1256: Imath's operator<< of a Vec4f
    std::cout << "[SolveDepthToDepth2] abcd:(" << k[0] << " " << k[1] << " " << k[2] << " " << k[3]
              << ") cost:" << sm[0] << "->" << sm[1] << std::endl;
    return true;
}

}  // namespace pff

namespace {
using namespace pff;

// Upload data[n], run `call` on the device copy in place, synchronise, download it back.
template <class Call>
void in_place(float* data, size_t n, const char* what, Call call)
{
    pf_ctx* c = facade_ctx();
    if (!c || !data) return;
    DevMem d(data, n);
    if (!d.ok || !call_sync(c, call(c, d.as<float>()), what)) return;
    download(data, d, n);
}

// ErrorData / ErrorEmap: the gt against a u16 result (given16) or a float map.  Like ErrorCompare
// and ErrorLaplacian below it downloads straight after the call: see download().
bool run_metrics(EquirectangularMap& gt, const float* given_f, const uint16_t* given16, int w,
                 int h, int given_c, int align_way, bool cap_depth, pf_metrics& m)
{
    pf_ctx* c = facade_ctx();
    if (!c || !gt.data) return false;
    const size_t n = (size_t)w * h;
    DevMem dg = on_device(gt), dv = given16 ? DevMem(given16, n) : DevMem(given_f, n * given_c),
           dm(sizeof(pf_metrics));
    if (!dg.ok || !dv.ok || !dm.ok) return false;
    return pf_ok(c, pf_error_metrics(c, dg.as<float>(), gt.width, gt.height, gt.channels,
                                     given16 ? nullptr : dv.as<float>(),
                                     given16 ? dv.as<uint16_t>() : nullptr, w, h, given_c, 1,
                                     g_zenith_range[0], g_zenith_range[1], align_way,
                                     cap_depth ? 1 : 0, dm.as<pf_metrics>()),
                 "pf_error_metrics") &&
           download(&m, dm, 1, "metrics download");
}

void fill(const pf_metrics& m, float& mse, float& mae, float& mre, float& mselog, float& d1,
          float& d2, float& d3, Vec2f* ls, float* shift)
{
    mse = m.mse;
    mae = m.mae;
    mre = m.mre;
    mselog = m.mselog;
    d1 = m.delta1;
    d2 = m.delta2;
    d3 = m.delta3;
    if (ls) *ls = Vec2f(m.ls_s, m.ls_o);
    if (shift) *shift = m.median_shift;
}

// The registration of SolveDepthToDepth / SolveDisparityToDepth: the emap and the maps `pm` on
// the device, `call` fits the four coefficients.
template <class Call>
bool solve(EquirectangularMap& emap, const std::vector<PerspectiveMap*>& pm, const char* what,
           Vec4f& abcd, Call call)
{
    pf_ctx* c = facade_ctx();
    if (!c || !emap.data) return false;
    DevMem dt = tiles_on_device(c, pm);
    if (!dt.ok) return false;
    DevMem de = on_device(emap), dc(4 * sizeof(float));
    if (!de.ok || !dc.ok) return false;
    float k[4];
    if (!pf_ok(c, call(c, de.as<float>(), dt.as<float>(), dc.as<float>()), what) ||
        !download(k, dc, 4))
        return false;
    abcd = to_vec4(k);
    return true;
}
}  // namespace

namespace DepthNamespace {

bool SetTileValidity(bool on, float lo, float hi)
{  // EXTENSION: pf_set_tile_validity for every later facade call
    if (on && !(lo < hi)) {
        std::cout << "[SetTileValidity] needs lo < hi (got " << lo << ", " << hi << ")"
                  << std::endl;
        return false;
    }
    std::lock_guard<std::mutex> lk(pff::g_rule_mu);
    pff::g_rule = pff::TileRule{on, on ? lo : 0.0f, on ? hi : 0.0f};
    return true;
}

bool SetRegistrationLoss(int kind, double a)
{  // EXTENSION: pf_set_register_loss for every later facade call
    const bool known = kind == PF_LOSS_NONE || kind == PF_LOSS_HUBER || kind == PF_LOSS_SOFTL1;
    if (!known || (kind != PF_LOSS_NONE && !(a > 0.0 && a < HUGE_VAL))) {
        std::cout << "[SetRegistrationLoss] needs PF_LOSS_NONE, or PF_LOSS_HUBER / PF_LOSS_SOFTL1 "
                     "with a finite scale a > 0 (got "
                  << kind << ", " << a << ")" << std::endl;
        return false;
    }
    std::lock_guard<std::mutex> lk(pff::g_rule_mu);
    pff::g_loss = pff::RegLossRule{kind, kind == PF_LOSS_NONE ? 0.0 : a};
    return true;
}

bool SetTileWeights(int mode, const std::string& suffix)
{  // EXTENSION: MergeDepthMaps registers and fuses with per-pixel tile weights
    pfw::Spec spec;
    std::string err;
    if (!pfw::make_spec(mode, suffix, spec, err)) {
        std::cout << "[SetTileWeights] " << err << std::endl;
        return false;
    }
    std::lock_guard<std::mutex> lk(pff::g_rule_mu);
    pff::g_tile_weights = spec;
    return true;
}

bool SetDisparityWeights(int mode, const std::string& arg)
{  // EXTENSION: MergeDisparityMaps fits and fuses with per-pixel weights
    pfdw::Spec spec;
    std::string err;
    if (!pfdw::make_spec(mode, arg, spec, err)) {
        std::cout << "[SetDisparityWeights] " << err << std::endl;
        return false;
    }
    std::lock_guard<std::mutex> lk(pff::g_rule_mu);
    pff::g_disp_weights = spec;
    return true;
}

bool SetTileDepth(int kind)
{  // EXTENSION: pf_set_tile_depth for every later facade call
    if (kind != PF_TILE_DEPTH_RAY && kind != PF_TILE_DEPTH_PLANAR) {
        std::cout << "[SetTileDepth] needs PF_TILE_DEPTH_RAY or PF_TILE_DEPTH_PLANAR (got " << kind
                  << ")" << std::endl;
        return false;
    }
    std::lock_guard<std::mutex> lk(pff::g_rule_mu);
    pff::g_tile_depth = kind;
    return true;
}

// ---- the four map members that run on the GPU ----
void EquirectangularMap::CopyInvalidPixels(EquirectangularMap& ref)  // Depth.cpp:703-725
{
    if (!facade_ctx() || !data || !ref.data) return;
    DevMem dr = on_device(ref);
    if (!dr.ok) return;
    in_place(data, count(*this), "pf_copy_invalid", [&](pf_ctx* c, float* d) {
        return pf_copy_invalid(c, d, width, height, channels, dr.as<float>(), ref.width,
                               ref.height, ref.channels, 1);
    });
}

void EquirectangularMap::DispDepthConversion()  // Depth.cpp:587-610
{
    in_place(data, count(*this), "pf_disp_depth_convert", [&](pf_ctx* c, float* d) {
        return pf_disp_depth_convert(c, d, (long long)width * height, channels);
    });
}

void PerspectiveMap::Depth2DepthTransform(Vec4f& abcd)
{
    const float k[4] = {abcd[0], abcd[1], abcd[2], abcd[3]};
    in_place(data, (size_t)width * height * channels, "pf_depth_transform",
             [&](pf_ctx* c, float* d) {
                 return pf_depth_transform(c, d, (long long)width * height, channels, k);
             });
}

void PerspectiveMap::D2DTransform(Vec4f abcd)  // Depth.cpp:214-243, on the GPU
{
    const float k[4] = {abcd[0], abcd[1], abcd[2], abcd[3]};
    in_place(data, (size_t)width * height * channels, "pf_disparity_transform",
             [&](pf_ctx* c, float* d) {
                 return pf_disparity_transform(c, d, (long long)width * height, channels, k);
             });
}

// ---- solvers ----
bool SolveDepthToDepth(EquirectangularMap& emap, std::vector<PerspectiveMap>& pmaps,
                       std::vector<bool>& actives, Vec2f& zr, Vec4f& abcd)
{
    // every active map's sample grid in one least-squares problem (Depth.cpp:1274-1376)
    const std::vector<PerspectiveMap*> pm = active_maps(pmaps, actives);
    if (pm.empty()) {
        std::cout << "[SolveDepthToDepth] no active map" << std::endl;
        return false;
    }
    const std::vector<int> all(pm.size(), 1);
    // under a loss (SetRegistrationLoss) one active map is the robust per-tile fit; several go to
    // the joint solve, which has no robust form and answers with the library's message.  The same
    // for planar-depth tiles (SetTileDepth): the per-tile fit carries the ray factor, the joint
    // solve does not.
    if (pm.size() == 1 &&
        (reg_loss().kind != PF_LOSS_NONE || tile_depth() != PF_TILE_DEPTH_RAY))
        return solve(emap, pm, "pf_register", abcd,
                     [&](pf_ctx* c, const float* de, float* dt, float* dc) {
                         return pf_register(c, de, emap.width, emap.height, emap.channels, dt, 1,
                                            zr[0], zr[1], 3, 0, dc, nullptr);
                     });
    return solve(emap, pm, "pf_register_joint", abcd,
                 [&](pf_ctx* c, const float* de, const float* dt, float* dc) {
                     return pf_register_joint(c, de, emap.width, emap.height, emap.channels, dt, 1,
                                              zr[0], zr[1], 3, all.data(), dc, nullptr);
                 });
}

// Depth.h:293-294 (declared there, never defined): y = 1/(a x + b) + d fitted to the one active
// map's samples (pf_register_disparity); abcd = (a, b, 1, d).
bool SolveDisparityToDepth(EquirectangularMap& emap, std::vector<PerspectiveMap>& pmaps,
                           std::vector<bool>& actives, Vec2f& zr, Vec4f& abcd)
{
    const std::vector<PerspectiveMap*> pm = active_maps(pmaps, actives);
    if (pm.size() != 1) {
        std::cout << "[SolveDisparityToDepth] needs exactly one active map (" << pm.size()
                  << " given): a joint disparity solve is not provided" << std::endl;
        return false;
    }
    return solve(emap, pm, "pf_register_disparity", abcd,
                 [&](pf_ctx* c, const float* de, float* dt, float* dc) {
                     return pf_register_disparity(c, de, emap.width, emap.height, emap.channels,
                                                  dt, 1, zr[0], zr[1], 0, dc, nullptr, nullptr);
                 });
}

// EXTENSION: every map's cubic fitted to the baseline and to its neighbours in the overlaps, one
// linear least-squares problem (pf_register_consistent); abcd_out[i] belongs to pmaps[i].
bool SolveDepthToDepthConsistent(EquirectangularMap& emap, std::vector<PerspectiveMap>& pmaps,
                                 Vec2f& zr, double lambda, std::vector<Vec4f>& abcd_out)
{
    pf_ctx* c = facade_ctx();
    if (!c || !emap.data) return false;
    if (pmaps.empty()) {
        std::cout << "[SolveDepthToDepthConsistent] no map" << std::endl;
        return false;
    }
    DevMem dt = tiles_on_device(c, pmaps);
    if (!dt.ok) return false;
    const size_t n = pmaps.size();
    DevMem de = on_device(emap), dc(4 * n * sizeof(float)), ds(4 * sizeof(double));
    if (!de.ok || !dc.ok || !ds.ok) return false;
    std::vector<float> k(4 * n);
    double sm[4];
    if (!pf_ok(c, pf_register_consistent(c, de.as<float>(), emap.width, emap.height, emap.channels,
                                         dt.as<float>(), 1, zr[0], zr[1], lambda, 0,
                                         dc.as<float>(), nullptr, ds.as<double>()),
               "pf_register_consistent") ||
        !download(k.data(), dc, 4 * n) || !download(sm, ds, 4))
        return false;
    if (sm[3] != 0.0) {
        std::cout << "[SolveDepthToDepthConsistent] the joint system is singular" << std::endl;
        return false;
    }
    abcd_out.resize(n);
    for (size_t i = 0; i < n; ++i) abcd_out[i] = to_vec4(&k[4 * i]);
    return true;
}

// EXTENSION: the statistics of the maps' disagreement on their overlaps (pf_overlap_stats), under
// abcds (one per map) or, with abcds empty, of the maps as they are.
bool TileOverlapStats(std::vector<PerspectiveMap>& pmaps, std::vector<Vec4f>& abcds, Vec2f& zr,
                      std::vector<TileOverlapStat>& stats_out)
{
    pf_ctx* c = facade_ctx();
    if (!c) return false;
    if (pmaps.empty() || (!abcds.empty() && abcds.size() != pmaps.size())) {
        std::cout << "[TileOverlapStats] needs maps, and no coefficients or one Vec4f per map"
                  << std::endl;
        return false;
    }
    DevMem dt = tiles_on_device(c, pmaps);
    if (!dt.ok) return false;
    int npairs = 0;
    long long nsamples = 0;
    if (!pf_ok(c, pf_overlap_pairs(c, zr[0], zr[1], &npairs, &nsamples), "pf_overlap_pairs"))
        return false;
    stats_out.clear();
    if (npairs == 0) return true;
    std::vector<float> k;
    for (const Vec4f& v : abcds) k.insert(k.end(), {v[0], v[1], v[2], v[3]});
    DevMem dk(k.data(), k.size()), dp(4 * (size_t)npairs * sizeof(int)),
        di(2 * (size_t)nsamples * sizeof(int)), ds(5 * (size_t)npairs * sizeof(double));
    if (!dk.ok || !dp.ok || !di.ok || !ds.ok) return false;
    std::vector<int> pairs(4 * (size_t)npairs);
    std::vector<double> st(5 * (size_t)npairs);
    if (!pf_ok(c, pf_overlap_table(c, zr[0], zr[1], dp.as<int>(), di.as<int>()),
               "pf_overlap_table") ||
        !pf_ok(c, pf_overlap_stats(c, dt.as<float>(), abcds.empty() ? nullptr : dk.as<float>(), 1,
                                   zr[0], zr[1], ds.as<double>()),
               "pf_overlap_stats") ||
        !download(pairs.data(), dp, pairs.size()) || !download(st.data(), ds, st.size()))
        return false;
    stats_out.resize(npairs);
    for (int i = 0; i < npairs; ++i)
        stats_out[i] = TileOverlapStat{pairs[4 * i], pairs[4 * i + 1], st[5 * i], st[5 * i + 1],
                                       st[5 * i + 2], st[5 * i + 3], st[5 * i + 4]};
    return true;
}

bool SolveDepthToDepth2(EquirectangularMap& emap, unsigned short* data, int width, int height,
                        Vec2f& zr, Vec4f& abcd)  // Depth.cpp:1158-1259
{
    pf_ctx* c = facade_ctx();
    if (!c || !emap.data || !data || width < 1 || height < 1) return false;
    DevMem de = on_device(emap), dd(data, (size_t)width * height);
    if (!de.ok || !dd.ok) return false;
    return global_fit(c, de.as<float>(), emap, dd.as<uint16_t>(), width, height, zr, false, abcd);
}

bool TransformResult(unsigned short* data, int width, int height, Vec2f& zr, Vec4f& abcd)
{
    pf_ctx* c = facade_ctx();
    if (!c || !data || width < 1 || height < 1) return false;
    const size_t no = (size_t)width * height;
    const float k[4] = {abcd[0], abcd[1], abcd[2], abcd[3]};
    DevMem dd(data, no), dc(k, 4);
    if (!dd.ok || !dc.ok) return false;
    return call_sync(c, pf_result_transform(c, dd.as<uint16_t>(), 1, width, height, zr[0], zr[1],
                                            dc.as<float>()),
                     "pf_result_transform") &&
           download(data, dd, no);
}

bool MedianScaling(EquirectangularMap& emap0, EquirectangularMap& emap1, float* emap0_median,
                   float* emap1_median)  // Depth.cpp:637-701
{
    auto any_valid = [](const EquirectangularMap& m) {
        if (!m.data) return false;
        const size_t n = (size_t)m.width * m.height;
        for (size_t i = 0; i < n; ++i) {
            const float v = m.data[i * m.channels];
            if (!(v < 1e-4 || v >= 1 - 1e-4) && v == v) return true;
        }
        return false;
    };
    if (!any_valid(emap0) || !any_valid(emap1)) {  // the reference indexes an empty vector here
        std::cout << "MedianScaling: zero val0_median ??" << std::endl;
        return false;
    }
    pf_ctx* c = facade_ctx();
    if (!c) return false;
    DevMem d0 = on_device(emap0), d1 = on_device(emap1), dm(2 * sizeof(float)), dst(sizeof(int));
    if (!d0.ok || !d1.ok || !dm.ok || !dst.ok) return false;
    if (!call_sync(c, pf_median_scale(c, d0.as<float>(), emap0.width, emap0.height, emap0.channels,
                                      d1.as<float>(), emap1.width, emap1.height, emap1.channels, 1,
                                      dm.as<float>(), dst.as<int>()),
                   "pf_median_scale"))
        return false;
    float med[2];
    int status = 0;
    if (!download(med, dm, 2) || !download(&status, dst, 1) || status != 0) return false;
    if (emap0_median) *emap0_median = med[0];
    if (emap1_median) *emap1_median = med[1];
    return download(emap0.data, d0, count(emap0));
}

bool SolveDepthAll(EquirectangularMap& emap, std::vector<PerspectiveMap>& pmaps,
                   unsigned short* data, int& out_width, int& out_height, Vec2f& zr,
                   const char* Laplacian_filename)
{
    (void)Laplacian_filename;  // debug dump of the targets in the reference; not produced
    pf_ctx* c = facade_ctx();
    if (!c || !emap.data) return false;
    const size_t no = (size_t)out_width * out_height;
    DevMem dt = tiles_on_device(c, pmaps);
    if (!dt.ok) return false;
    DevMem de = on_device(emap), dout(no * 2);
    if (!de.ok || !dout.ok) return false;
    // PF_ETIMEOUT from the synchronisation: invalid output
    return call_sync(c, pf_fuse(c, de.as<float>(), emap.width, emap.height, emap.channels,
                                dt.as<float>(), nullptr, 1, out_width, out_height, zr[0], zr[1],
                                dout.as<uint16_t>()),
                     "pf_fuse") &&
           download(data, dout, no);
}

bool SolveDepthBySmoothing(std::vector<PerspectiveMap>& pmaps, unsigned short* data,
                           int& out_width, int& out_height, Vec2f& zr)
{  // Depth.cpp:1773-1878 on the GPU (pf_solve_smoothing)
    pf_ctx* c = facade_ctx();
    if (!c) return false;
    const size_t no = (size_t)out_width * out_height;
    DevMem dt = tiles_on_device(c, pmaps), dout(dt.ok ? no * 2 : 0);
    if (!dt.ok || !dout.ok) return false;
    // a row-band hand-off that timed out makes the result invalid: the synchronisation reports
    // it here, on this call (PF_ETIMEOUT), as SolveDepthAll's does for the fusion
    return call_sync(c, pf_solve_smoothing(c, dt.as<float>(), nullptr, 1, out_width, out_height,
                                           zr[0], zr[1], dout.as<uint16_t>()),
                     "pf_solve_smoothing", "SolveDepthBySmoothing") &&
           download(data, dout, no);
}

bool StitchDepthMaps(std::vector<PerspectiveMap>& pmaps, unsigned short* data, int& width,
                     int& height)
{  // EXTENSION: Depth.cpp:817-865 on the GPU (pf_stitch), the tiles as they are
    pf_ctx* c = facade_ctx();
    if (!c || !data) return false;
    const size_t no = (size_t)width * height;
    DevMem dt = tiles_on_device(c, pmaps), dout(dt.ok ? no * 2 : 0);
    if (!dt.ok || !dout.ok) return false;
    return call_sync(c, pf_stitch(c, dt.as<float>(), nullptr, 1, width, height,
                                  dout.as<uint16_t>()),
                     "pf_stitch") &&
           download(data, dout, no);
}

bool CheckLaplacian(EquirectangularMap& emap, std::vector<PerspectiveMap>& pmaps, int width,
                    int height, Vec2f& zr, std::vector<float>& err_per_level)
{  // EXTENSION: Depth.cpp:1738-1758 on the GPU, after every level (pf_fuse_check)
    pf_ctx* c = facade_ctx();
    if (!c || !emap.data) return false;
    DevMem dt = tiles_on_device(c, pmaps);
    if (!dt.ok) return false;
    int nlevels = 0;
    if (!pf_ok(c, pf_level_info(width, height, zr[0], zr[1], 0, nullptr, nullptr, nullptr, nullptr,
                                nullptr, &nlevels),
               "pf_level_info") ||
        nlevels < 1)
        return false;
    DevMem de = on_device(emap), derr(sizeof(float) * nlevels);
    if (!de.ok || !derr.ok) return false;
    // PF_ETIMEOUT from the synchronisation: invalid planes
    if (!call_sync(c, pf_fuse_check(c, de.as<float>(), emap.width, emap.height, emap.channels,
                                    dt.as<float>(), nullptr, width, height, zr[0], zr[1],
                                    derr.as<float>(), nullptr),
                   "pf_fuse_check"))
        return false;
    err_per_level.assign(nlevels, 0.0f);
    return download(err_per_level.data(), derr, nlevels);
}

// ---- ErrorData / ErrorEmap (Depth.cpp:1960-2458) ----
bool ErrorData(EquirectangularMap& gt, unsigned short* data, int w, int h, float& mse,
               float& mae, float& mre, float& mselog, float& d1, float& d2, float& d3,
               int align_way, bool cap_depth, Vec2f* ls, float* shift)
{
    pf_metrics m;
    if (!run_metrics(gt, nullptr, data, w, h, 1, align_way, cap_depth, m)) return false;
    fill(m, mse, mae, mre, mselog, d1, d2, d3, ls, shift);
    return true;
}

bool ErrorEmap(EquirectangularMap& gt, EquirectangularMap& given, float& mse, float& mae,
               float& mre, float& mselog, float& d1, float& d2, float& d3, int align_way,
               bool cap_depth, Vec2f* ls, float* shift)
{
    pf_metrics m;
    if (!run_metrics(gt, given.data, nullptr, given.width, given.height, given.channels,
                     align_way, cap_depth, m))
        return false;
    fill(m, mse, mae, mre, mselog, d1, d2, d3, ls, shift);
    return true;
}

// ---- ErrorCompare (Depth.cpp:2460-2634) ----
bool ErrorCompare(EquirectangularMap& emap_gt, EquirectangularMap& emap_baseline,
                  bool DispDepthCompare, float& mse, float& mae, float& mre, float& mselog,
                  float& delta1, float& delta2, float& delta3, int align_way, bool cap_depth,
                  Vec2f* fit, Vec2f* minmax, std::vector<unsigned char>* shifted, int* n_nonblack)
{
    EquirectangularMap &gt = emap_gt, &given = emap_baseline;
    pf_ctx* c = facade_ctx();
    if (!c || !gt.data || !given.data) return false;
    const size_t npx = (size_t)given.width * given.height;
    DevMem dg = on_device(gt), dv = on_device(given), dr(sizeof(pf_compare)),
           ds(shifted ? npx : 0);  // the 8-bit plane, when it is asked for
    if (!dg.ok || !dv.ok || !dr.ok || !ds.ok) return false;
    pf_compare r;
    if (!pf_ok(c, pf_error_compare(c, dg.as<float>(), gt.width, gt.height, gt.channels,
                                   dv.as<float>(), given.width, given.height, given.channels, 1,
                                   g_zenith_range[0], g_zenith_range[1], DispDepthCompare ? 1 : 0,
                                   align_way, cap_depth ? 1 : 0, dr.as<pf_compare>(), nullptr,
                                   shifted ? ds.as<uint8_t>() : nullptr),
               "pf_error_compare") ||
        !download(&r, dr, 1, "compare download"))
        return false;
    if (shifted) {
        shifted->resize(npx);
        if (!download(shifted->data(), ds, npx, "shifted download")) return false;
    }
    fill(r.m, mse, mae, mre, mselog, delta1, delta2, delta3, nullptr, nullptr);
    if (fit) *fit = Vec2f(r.fit_s, r.fit_o);
    if (minmax) *minmax = Vec2f(r.vmin, r.vmax);
    if (n_nonblack) *n_nonblack = r.n_nonblack;
    return true;
}

bool ErrorCompare(std::string& gt_filename, std::string& baseline_filename, bool DispDepthCompare,
                  float& mse, float& mae, float& mre, float& mselog, float& delta1, float& delta2,
                  float& delta3, int align_way, bool cap_depth, const char* shifted_filename)
{
    EquirectangularMap emap_gt, emap_baseline;
    if (!load_pair(gt_filename, baseline_filename, true /*mono360*/, emap_gt, emap_baseline))
        return false;
    Vec2f minmax;
    std::vector<unsigned char> shifted;
    if (!ErrorCompare(emap_gt, emap_baseline, DispDepthCompare, mse, mae, mre, mselog, delta1,
                      delta2, delta3, align_way, cap_depth, nullptr, &minmax,
                      shifted_filename ? &shifted : nullptr))
        return false;
    if (DispDepthCompare)  // Depth.cpp:2552
        std::cout << "DispDepthCompare emap_baseline minmax:(" << minmax[0] << " " << minmax[1]
                  << ")" << std::endl;
    if (shifted_filename) {
        // stbi_write_png's return value: 1 on success, 0 on failure
        const int ret = Save8BitPNG(shifted.data(), emap_baseline.width, emap_baseline.height,
                                    shifted_filename) ? 1 : 0;
        std::cout << "[ErrorCompare] " << ret << " saved shifted emap:" << shifted_filename
                  << std::endl;  // Depth.cpp:2599, :2628
    }
    return true;
}

// ---- ErrorLaplacian (Depth.cpp:2636-2953) ----
bool ErrorLaplacian(EquirectangularMap& emap_gt, EquirectangularMap& emap_baseline,
                    double& Laplacian_mse, double& Laplacian_mae, double& SobelX_mae,
                    double& SobelY_mae, double& Laplacian5x5_mae, long long* counts)
{
    EquirectangularMap &gt = emap_gt, &given = emap_baseline;
    pf_ctx* c = facade_ctx();
    if (!c || !gt.data || !given.data) return false;
    DevMem dg = on_device(gt), dv = on_device(given), dm(sizeof(pf_edge_metrics));
    if (!dg.ok || !dv.ok || !dm.ok) return false;
    pf_edge_metrics m;
    if (!pf_ok(c, pf_error_laplacian(c, dg.as<float>(), gt.width, gt.height, gt.channels,
                                     dv.as<float>(), nullptr, given.width, given.height,
                                     given.channels, 1, dm.as<pf_edge_metrics>(), nullptr, nullptr,
                                     nullptr),
               "pf_error_laplacian") ||
        !download(&m, dm, 1, "edge metrics download"))
        return false;
    Laplacian_mse = m.lap_mse;
    Laplacian_mae = m.lap_mae;
    SobelX_mae = m.sobelx_mae;
    SobelY_mae = m.sobely_mae;
    Laplacian5x5_mae = m.lap5_mae;
    if (counts) {
        counts[0] = m.n_lap;
        counts[1] = m.n_sobel;
        counts[2] = m.n_lap5;
    }
    std::cout << "[ErrorLap] Lap_mse:" << Laplacian_mse << " Lap_mae:" << Laplacian_mae
              << " SobelX:" << SobelX_mae << " SobelY:" << SobelY_mae
              << " Lap5x5:" << Laplacian5x5_mae << std::endl;  // Depth.cpp:2950-2951
    return true;
}

bool ErrorLaplacian(std::string& gt_filename, std::string& baseline_filename,
                    double& Laplacian_mse, double& Laplacian_mae, double& SobelX_mae,
                    double& SobelY_mae, double& Laplacian5x5_mae, std::string*, std::string*,
                    std::string*)
{
    EquirectangularMap emap_gt, emap_baseline;
    if (!load_pair(gt_filename, baseline_filename, false, emap_gt, emap_baseline)) return false;
    return ErrorLaplacian(emap_gt, emap_baseline, Laplacian_mse, Laplacian_mae, SobelX_mae,
                          SobelY_mae, Laplacian5x5_mae);
}

}  // namespace DepthNamespace
