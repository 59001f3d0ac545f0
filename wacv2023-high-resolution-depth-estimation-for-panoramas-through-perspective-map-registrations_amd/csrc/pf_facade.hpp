// pf_facade.hpp -- what the GPU units of the DepthNamespace facade share (pf_depth_gpu.cpp,
// pf_depth_merge.cpp, pf_depth_mode0.cpp): the per-device context, device memory that frees
// itself, the two error checks and the few steps every entry point is made of.  Private to
// libpanofuse_depth.so and its command line (pf_main.cpp uses the inline helpers only); the
// host-only maps unit (pf_depth_maps.cpp) does not include it.
#pragma once

#include "../../include/pf_depth.h"
#include "../../include/panofuse.h"
#include "pf_disp_weights.hpp"
#include "pf_weights.hpp"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <iostream>
#include <string>
#include <utility>

// hidden: nothing in pff is an export of the library
namespace pff __attribute__((visibility("hidden"))) {

using DepthNamespace::EquirectangularMap;
using DepthNamespace::PerspectiveMap;

// One context per device, created on first use (the reference is single-threaded and not
// re-entrant; so is this facade per device).  PF_METRICS_ORDER is read here, once per context.
pf_ctx* facade_ctx();

// The tile-pixel validity rule of the facade (SetTileValidity): process-wide, and put on the
// context every time facade_ctx() hands it out, so every entry point starts from it.
struct TileRule {
    bool on;
    float lo, hi;
};
TileRule tile_rule();
inline int apply_rule(pf_ctx* c, const TileRule& r)
{
    return pf_set_tile_validity(c, r.on ? PF_VALID_RANGE : PF_VALID_ALL, r.lo, r.hi);
}

// The robust registration loss of the facade (SetRegistrationLoss), carried the same way.
struct RegLossRule {
    int kind;  // PF_LOSS_*
    double a;
};
RegLossRule reg_loss();
inline int apply_loss(pf_ctx* c, const RegLossRule& r)
{
    return pf_set_register_loss(c, r.kind, r.a);
}
// What the tiles hold (SetTileDepth): PF_TILE_DEPTH_*, carried the same way.
int tile_depth();
// The per-pixel tile weights of MergeDepthMaps (SetTileWeights), carried the same way.
pfw::Spec tile_weights();
// The disparity tiles' weights of MergeDisparityMaps (SetDisparityWeights), carried the same way.
pfdw::Spec disparity_weights();
// "huber:A" or "softl1:A" with a finite A > 0 (PF_REG_LOSS / --reg-loss).
inline bool parse_reg_loss(const char* s, RegLossRule& r)
{
    const std::string v(s ? s : "");
    const size_t colon = v.find(':');
    if (colon == std::string::npos) return false;
    const std::string name = v.substr(0, colon), num = v.substr(colon + 1);
    if (name == "huber") r.kind = PF_LOSS_HUBER;
    else if (name == "softl1") r.kind = PF_LOSS_SOFTL1;
    else return false;
    char* end = nullptr;
    r.a = std::strtod(num.c_str(), &end);
    return !num.empty() && end && *end == '\0' && r.a > 0.0 && r.a < HUGE_VAL;
}

inline bool hip_ok(hipError_t e, const char* what)
{
    if (e == hipSuccess) return true;
    std::cout << "[panofuse] " << what << ": " << hipGetErrorString(e) << std::endl;
    return false;
}

inline bool pf_ok(pf_ctx* c, int rc, const char* what)
{
    if (rc == PF_OK) return true;
    std::cout << "[panofuse] " << what << " failed (" << rc << "): " << pf_last_error(c)
              << std::endl;
    return false;
}

// Call, check, synchronise.  pf_synchronize is where a fusion whose row-band hand-off timed out
// reports PF_ETIMEOUT (an invalid output), under the name `sync_what`.
inline bool call_sync(pf_ctx* c, int rc, const char* what, const char* sync_what = "pf_synchronize")
{
    return pf_ok(c, rc, what) && pf_ok(c, pf_synchronize(c), sync_what);
}

struct DevMem {
    void* p = nullptr;
    bool ok = true;
    explicit DevMem(size_t bytes) { ok = bytes == 0 || hipMalloc(&p, bytes) == hipSuccess; }
    // a device copy of the host array h[n]
    template <class T>
    DevMem(const T* h, size_t n) : DevMem(n * sizeof(T))
    {
        ok = ok && hip_ok(hipMemcpy(p, h, n * sizeof(T), hipMemcpyHostToDevice), "upload");
    }
    ~DevMem()
    {
        if (p) (void)hipFree(p);
    }
    DevMem(DevMem&& o) noexcept : p(std::exchange(o.p, nullptr)), ok(o.ok) {}
    DevMem(const DevMem&) = delete;
    DevMem& operator=(const DevMem&) = delete;
    template <class T>
    T* as() const { return (T*)p; }
};

// Download n values of T.  It is a blocking hipMemcpy on the null stream, which is the stream the
// facade's contexts run on (pf_set_stream is never called): it starts after every kernel the
// preceding pf_* call enqueued.  pf_error_metrics, pf_error_compare and pf_error_laplacian only
// launch kernels on that stream (pf_eval.hip) and have no timeout to report, so run_metrics,
// run_compare and run_edge download straight after the call, without pf_synchronize.
template <class T>
bool download(T* h, const DevMem& d, size_t n, const char* what = "download")
{
    return hip_ok(hipMemcpy(h, d.p, n * sizeof(T), hipMemcpyDeviceToHost), what);
}

inline size_t count(const EquirectangularMap& m) { return (size_t)m.width * m.height * m.channels; }
inline DevMem on_device(const EquirectangularMap& m) { return DevMem(m.data, count(m)); }

inline pf_window to_window(const Vec4f& v) { return pf_window{v[0], v[1], v[2], v[3]}; }
inline Vec4f to_vec4(const float k[4]) { return Vec4f(k[0], k[1], k[2], k[3]); }

// The maps as the tile layout of the context (windows, ranges as stored in the maps, sizes) and
// channel 0 of every map, tile after tile, on the device.  !ok after a message when a map has no
// data or no window, or when pf_set_tiles refuses the layout.
DevMem tiles_on_device(pf_ctx* c, const std::vector<PerspectiveMap*>& pm);
DevMem tiles_on_device(pf_ctx* c, std::vector<PerspectiveMap>& pmaps);  // all of them
// The maps whose `actives` entry is set, for the list form above.
std::vector<PerspectiveMap*> active_maps(std::vector<PerspectiveMap>& pmaps,
                                         const std::vector<bool>& actives);

// The fused u16 result on the device registered to the baseline by SolveDepthToDepth2's cubic
// (pf_register_global; apply: transformed as well); prints the "[SolveDepthToDepth2] ..." line.
bool global_fit(pf_ctx* c, const float* d_emap, const EquirectangularMap& emap, uint16_t* d_data,
                int w, int h, Vec2f& zr, bool apply, Vec4f& abcd);

// gt.Load(gt_fn) and given.Load(given_fn, mono360) with the reference's two lines for a file that
// does not load (Depth.cpp:2474-2484, :2650-2660).
inline bool load_pair(std::string& gt_fn, std::string& given_fn, bool mono360,
                      EquirectangularMap& gt, EquirectangularMap& given)
{
    if (!gt.Load(gt_fn)) {
        std::cout << "cannot load emap_gt? " << gt_fn << std::endl;
        return false;
    }
    if (!given.Load(given_fn, mono360)) {
        std::cout << "cannot load emap_baseline? " << given_fn << std::endl;
        return false;
    }
    return true;
}

// The export's tile size for a window (SaveCubeMap's viewport), pf_depth_mode0.cpp.
void rgb_tile_size(const Vec4f& fov, int& w, int& h);

}  // namespace pff
