// pf_ctx.hpp -- private to the host units of libpanofuse (pf_ctx.hip, pf_layout.hip, pf_plan.hip,
// pf_fuse.hip, pf_shard.hip, pf_warp_api.hip, pf_smooth_api.hip, pf_eval.hip, pf_disp_api.hip,
// pf_global_api.hip, pf_stitch_api.hip, pf_consist_api.hip, pf_weight_api.hip): the context struct
// behind the C-ABI's opaque pf_ctx, the error / allocation / upload helpers, the argument-check
// prologues the entry points share, and the few functions that cross those units.  No kernel unit
// includes it.
#pragma once
#include "../../include/panofuse.h"
#include "pf_internal.hpp"

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace pf {

// A device allocation owned by the context (grown by ensure()); freed with it.
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf()
    {
        if (p) (void)hipFree(p);
    }
};

struct LevelCache {
    int out_w = 0, out_h = 0;  // out_w == 0: invalid (pf_set_tiles, a failed prepare_levels)
    uint32_t zr0 = 0, zr1 = 0;
    int nlevels = 0;
    LevelDims dims[4];
    DevBuf box[4], cols[4], rows[4], tapbox[4], tapmap[4], hcol[4];
    DevBuf tmask[4];  // per targets patch, the tiles whose box meets it (k_targets_multi)
    // (pixel, tile) pairs of the pixels covered by three or more tiles, sorted by pixel then
    // tile (the sharded fusion recomputes their sums in tile order: pf_fuse_multicover)
    DevBuf mcpairs[4];
    int nmc[4] = {0, 0, 0, 0};
    std::vector<TileBox> box_h[4];
    // separable-coverage certificate of each level: a band pixel is covered iff it lies in rows
    // h0+1..h1-1 and in a column of a fixed set that excludes column 0.  Enables the packed
    // Jacobi form (pf_jacobi.hip), with hcol[l][X] = 0.5 on covered columns, 0 elsewhere.
    bool full[4] = {false, false, false, false};
    // tap-grid points of each level (one tile texel gathered per point): the targets stage's
    // algorithmic read count
    long long taps[4] = {0, 0, 0, 0};
    // the one-launch targets of every level (k_targets_multi): (level, patch) gather order
    DevBuf tgt_order;
    int tgt_nentries = 0;
};

}  // namespace pf

struct pf_ctx {
    int device = 0;
    int num_cu = 256;
    hipStream_t stream = nullptr;
    std::string err;
    // layout
    int ntiles = 0, tile_c = 1;
    int solver = PF_SOLVER_LM;  // degree-3 registration solver (pf_set_solver)
    int metrics_order = PF_METRICS_TREE;  // pf_set_metrics_order
    // tile-pixel validity rule (pf_set_tile_validity); valid.on == 0: every pixel is read
    pf::TileValid valid{0, 0.0f, 0.0f};
    // robust loss of the tile registrations (pf_set_register_loss); PF_LOSS_NONE: least squares
    int loss_kind = PF_LOSS_NONE;
    double loss_a = 0.0;
    // what the tiles hold (pf_set_tile_depth); PF_TILE_DEPTH_RAY: ray distance, as the reference
    // assumes, and every entry point launches what it always did
    int tile_depth = PF_TILE_DEPTH_RAY;
    // per-pixel tile weights of the weighted call that is running (pf_fuse_weighted,
    // pf_merge_weighted; pf_weight_api.hip sets and clears them): the device plane in the tiles'
    // element layout and its panorama stride (0: one set for the batch).  nullptr: no weights,
    // and the fusion gathers what it always did
    const float* wts = nullptr;
    long long wts_stride = 0;
    std::vector<pf_window> fov, rng;
    std::vector<int> tw_h, th_h;
    bool layout_ok = false;  // the stored layout was set completely
    std::vector<pf::TileGeom> geom_h;
    std::vector<pf::RegGrid> reg_h;
    long long tile_elems = 0, npix_max = 0, rgb_elems = 0;
    pf::DevBuf geom, reg, rcols, rrows, rgb_off;
    pf::DevBuf reg_sidx;                   // registration sample indices (k_regidx), for the
    int reg_sidx_key[3] = {-1, -1, -1};    // (ew, eh, ec) of the baseline they were built for
    // the ray factor of planar-depth tiles: the layout's fp64 column / row tables (pf_ray.hpp; host
    // copy and device copy, uploaded by pf_set_tiles), where each tile's start, and the factor of
    // every registration sample (k_reg_kf), built on first planar use for the key of reg_sidx
    std::vector<double> ray_tab_h;
    std::vector<pf::RayTile> ray_h;
    pf::DevBuf ray_tab, ray, reg_kf;
    int reg_kf_key[3] = {-1, -1, -1};
    // the tile-pair overlap table (pf_consist_api.hip) of the registration grids: the pair list
    // {p, q, first, count} (host copy and device copy) and the samples' {element in p, element in
    // q}; rebuilt when the grids are (prepare_registration drops it).  Then the pair moment sums,
    // the statistics and the solve's global workspace of pf_register_consistent.
    bool pair_valid = false;
    std::vector<int> pairs_h;
    long long pair_samples = 0;
    pf::DevBuf pair_counts, pair_list, pair_index, pair_sums, consist_ws;
    std::vector<pf::RgbCam> cams_h;  // GL cameras of the RGB warp (SaveCubeMap), host only
    // RGB warp taps for one panorama size (rgb_taps_host), built on first use
    int rgb_pw = 0, rgb_ph = 0;
    pf::DevBuf rgbtap;
    // LDS-staged RGB warp (k_warp_rgb_box): patch boxes, per-pixel box index and weights
    pf::DevBuf rgbpatch, rgbunits, rgbloc, rgbw;
    int n_rgbpatch = 0;
    bool rgb_staged = false;
    pf::LevelCache lc;
    bool reg_valid = false;
    uint32_t reg_zr0 = 0, reg_zr1 = 0;
    // E->P depth warp for one panorama size (pf_warp.hip): tile patches with their panorama
    // boxes, per tile pixel the corner index in its box and the (fx, fy) weights; built on
    // first use
    int wmap_pw = 0, wmap_ph = 0, npatch = 0;
    pf::DevBuf wmap, wfxy, wpatch, wunits;  // wunits: the ragged footprints' unit table
    std::vector<pf::WarpPatch> wpatch_grid_h;  // the layout's plain 64x32 patch grid
    // workspace
    pf::DevBuf buf[3], lnorm, coeffs, lsum_ws, metrics_ws, reg_sums, reg_active;
    pf::DevBuf audit_ws;    // pf_layout_audit: the counter words
    // pf_merge_disparity, pf_merge under PF_TILE_DEPTH_PLANAR: the transformed copy of the
    // caller's tiles
    pf::DevBuf disp_tiles;
    // pf_register_disparity_weighted: the samples' usable weights, [batch][samples] floats in
    // sample order (k_disp_sample_weights), rewritten by every call
    pf::DevBuf disp_ws;
    // pf_register_global: ValueAtCoord's column / row terms for one (result size, baseline size)
    // key, the chunk partials with the coefficients after them; pf_median_scale: bins and states
    pf::DevBuf glob_ecol, glob_erow, glob_ws, med_ws;
    int glob_key[5] = {0, 0, 0, 0, 0};
    // pf_error_compare: the fit's and the final call's pf_metrics, the min / max cells, the gt
    // disparity plane and (when the caller passes none) the depth plane; apart from metrics_ws,
    // which the two inner pf_error_metrics calls size for themselves
    pf::DevBuf cmp_ws;
    // SolveDepthBySmoothing (pf_smooth.hip): boxes, grid tables, per-pixel source and mask
    pf::DevBuf sm_box, sm_cols, sm_rows, sm_src, sm_mask;
    // its compacted pixel list (k_smooth_iter_list), cached for one (boxes, size, band) key
    pf::DevBuf sm_list, sm_off;
    std::vector<pf::SmoothBox> sm_key_boxes;
    int sm_key[4] = {0, 0, 0, 0}, sm_nk = 0, sm_nb = 0, sm_smin = 0, sm_smax = -1;
    // row-band smoothing (k_smooth_band): ticket, timeouts, per-block step flags
    pf::DevBuf sm_sync;
    uint32_t sm_tk = 0, sm_fb = 1;
    // the direct stitch (pf_stitch.hip): boxes, grid tables and the per-pixel (first covering
    // tile, Value index) map of one output size (st_key; pf_set_tiles drops it)
    pf::DevBuf st_box, st_cols, st_rows, st_src;
    int st_key[2] = {0, 0};
    // level-0 seed index tables of the streaming Jacobi (seed_tables), keyed by level and emap
    pf::DevBuf seed_ecol, seed_erow;
    // resident level kernel (pf_jres.hip): hand-off rows, and the sync words ([0] ticket
    // counter, [1] spin timeouts, [2..] one flag per row block); tickets and flags are
    // monotone across launches (jres_tk, jres_fb), so nothing is reset between launches
    pf::DevBuf jres_x, jres_sync;
    uint32_t jres_tk = 0, jres_fb = 1;
    int jres_mode = -1, jres_nb = 0;  // pf_set_jacobi_engine (-1: not set, PF_JRES decides)
    double jacobi_share = 1.0;  // pf_set_jacobi_share: the chip share the pass plans assume
    // timeout reporting: a resident launch whose wait times out also raises this flag in
    // coherent pinned host memory (a system-scope store from the kernel, no extra stream work);
    // jres_check reports a raised flag once as PF_ETIMEOUT and lowers it
    uint32_t* jres_err_h = nullptr;
    int jres_fault = 0;  // pf_debug_jres_fault: spin_log2 for the next resident launch (0: off)
    int smooth_fault = 0;  // pf_debug_smooth_fault: spin_log2 for the next row-band smoothing
    int seed_key[5] = {0, 0, 0, 0, 0};
    // stage profiling
    struct Span {
        int stage;
        hipEvent_t a, b;
        double bytes;
        long long launches;
    };
    bool prof_on = false;
    std::vector<Span> spans;
    std::vector<hipEvent_t> event_pool;
    // end of each level's sweeps in the last fusion (pf_stream_wait_level), created on first use
    hipEvent_t ev_level[4] = {};
    int nlev_recorded = 0;
};

namespace pf {

inline hipEvent_t take_event(pf_ctx* c)
{
    if (!c->event_pool.empty()) {
        hipEvent_t e = c->event_pool.back();
        c->event_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

// Records an event pair around a stage when profiling is on (RAII: end on scope exit).
struct StageTimer {
    pf_ctx* c;
    long idx = -1;
    StageTimer(pf_ctx* c_, int stage, double bytes, long long launches) : c(c_)
    {
        if (!c->prof_on) return;
        pf_ctx::Span s{stage, take_event(c), take_event(c), bytes, launches};
        (void)hipEventRecord(s.a, c->stream);
        c->spans.push_back(s);
        idx = (long)c->spans.size() - 1;
    }
    ~StageTimer()
    {
        if (idx >= 0) (void)hipEventRecord(c->spans[idx].b, c->stream);
    }
    void set_launches(long long n)
    {
        if (idx >= 0) c->spans[idx].launches = n;
    }
};

// ---------------------------------------------------------------------------------------------
inline int fail(pf_ctx* c, int code, const char* fmt, ...)
{
    char msg[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, sizeof(msg), fmt, ap);
    va_end(ap);
    if (c) c->err = msg;
    return code;
}

#define HIPCHK(ctx, expr)                                                                    \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return fail(ctx, PF_EHIP, "%s: %s", #expr, hipGetErrorString(e_));               \
    } while (0)

inline int ensure(pf_ctx* c, DevBuf& b, size_t bytes)
{
    if (b.bytes >= bytes) return PF_OK;
    if (b.p) {
        (void)hipStreamSynchronize(c->stream);
        (void)hipFree(b.p);
        b.p = nullptr;
        b.bytes = 0;
    }
    if (bytes == 0) return PF_OK;
    if (hipMalloc(&b.p, bytes) != hipSuccess)
        return fail(c, PF_ENOMEM, "hipMalloc(%zu) failed", bytes);
    b.bytes = bytes;
    return PF_OK;
}

template <class T>
int upload(pf_ctx* c, DevBuf& b, const std::vector<T>& v)
{
    int rc = ensure(c, b, v.size() * sizeof(T) + 16);
    if (rc) return rc;
    if (!v.empty())
        HIPCHK(c, hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice,
                                 c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // host vector may die after return
    return PF_OK;
}

// ---- prologues of the entry points ----------------------------------------------------------
inline int check_common(pf_ctx* c, int batch)
{
    if (!c) return PF_EINVAL;
    if (c->ntiles <= 0) return fail(c, PF_ESTATE, "no tile layout: call pf_set_tiles first");
    if (batch <= 0 || batch > 65535) return fail(c, PF_EINVAL, "batch %d out of range", batch);
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, PF_EHIP, "hipSetDevice failed");
    return PF_OK;
}

// The evaluation entries need no tile layout: the context and its device only.
inline int check_device(pf_ctx* c)
{
    if (!c) return PF_EINVAL;
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, PF_EHIP, "hipSetDevice failed");
    return PF_OK;
}

inline int check_emap(pf_ctx* c, const float* emap, int ew, int eh, int ec)
{
    if (!emap || ew < 2 || eh < 2 || ec < 1)
        return fail(c, PF_EINVAL, "bad emap %p %dx%dx%d", (const void*)emap, ew, eh, ec);
    if ((long long)ew * eh * ec >= (1LL << 31))  // 32-bit emap indices (seed_tables, pf_fuse.hip)
        return fail(c, PF_EINVAL, "emap %dx%dx%d too large", ew, eh, ec);
    return PF_OK;
}

// The entry points that cannot honour the tile-pixel validity rule refuse to run under it.
inline int check_unmasked(pf_ctx* c, const char* entry)
{
    if (c && c->valid.on)
        return fail(c, PF_ESTATE,
                    "%s does not honour the tile validity rule: call pf_set_tile_validity(ctx, "
                    "PF_VALID_ALL, 0, 0) first",
                    entry);
    return PF_OK;
}

// The entry points that have no robust form refuse to run while a loss is set.
inline int check_no_loss(pf_ctx* c, const char* entry)
{
    if (c && c->loss_kind != PF_LOSS_NONE)
        return fail(c, PF_ESTATE,
                    "%s has no robust form: call pf_set_register_loss(ctx, PF_LOSS_NONE, 0) first",
                    entry);
    return PF_OK;
}

// The entry points whose fused-transform gathers have no ray factor refuse coefficients while the
// tiles are planar depth (without coefficients the tiles are read as they are: ray distance).
inline int check_ray_coeffs(pf_ctx* c, const char* entry, const void* coeffs)
{
    if (c && c->tile_depth != PF_TILE_DEPTH_RAY && coeffs)
        return fail(c, PF_ESTATE,
                    "%s has no ray factor in its fused transform: register with apply (or pf_merge) "
                    "and pass coeffs = NULL, or call pf_set_tile_depth(ctx, PF_TILE_DEPTH_RAY) "
                    "first",
                    entry);
    return PF_OK;
}

// Whether level l may take the coverage shortcuts (the packed Jacobi form, the resident kernel):
// it holds the separable-coverage certificate and coverage does not depend on the data (it does
// under the validity rule and under per-pixel weights).
inline bool level_full(const pf_ctx* c, int l)
{
    return c->lc.full[l] && !c->valid.on && !c->wts;
}

inline int check_tile_range(pf_ctx* c, int t0, int t1)
{
    if (t0 < 0 || t1 > c->ntiles || t0 > t1)
        return fail(c, PF_EINVAL, "tile range [%d,%d) outside [0,%d)", t0, t1, c->ntiles);
    return PF_OK;
}

// ---- pf_layout.hip --------------------------------------------------------------------------
// The level cache (c->lc) for this output size and zenith range, rebuilt when they change.
int prepare_levels(pf_ctx* c, int out_w, int out_h, float zr0, float zr1);
// The registration grids for this zenith range, and the checks / tables that follow them.
int prepare_registration(pf_ctx* c, float zr0, float zr1);
const int2* reg_sample_index(pf_ctx* c, int ew, int eh, int ec);
// The ray factor of the samples of reg_sample_index(c, ew, eh, ec) (nullptr: no table).
const float* reg_sample_kf(pf_ctx* c, int ew, int eh, int ec);
int check_reg_grids(pf_ctx* c, const int* active);
void grid_tables(const LevelDims& L, std::vector<GridCol>& cols, std::vector<GridRow>& rows);

// The level prologue: the level cache, then the level-range check; *L = the level's dimensions.
inline int level_at(pf_ctx* c, int out_w, int out_h, float zr0, float zr1, int level,
                    const LevelDims** L)
{
    int rc;
    if ((rc = prepare_levels(c, out_w, out_h, zr0, zr1))) return rc;
    if (level < 0 || level >= c->lc.nlevels) return fail(c, PF_EINVAL, "bad level %d", level);
    *L = &c->lc.dims[level];
    return PF_OK;
}

// ---- pf_plan.hip: the planners (no stream work) ---------------------------------------------
struct PassPlan {
    int T = 1, nchunks = 1;
    int stages = 1;  // > 1: the pipelined engine (k_jpipe), T/stages levels per wave
    double cost = 0;
};

// The resident level kernel (pf_jres.hip): one launch for all of a level's sweeps, for the
// widths it is built for (a wave holds whole rows) and levels with the packed-form certificate.
// nb row blocks per panorama of `core` rows; every K sweeps the blocks trade K halo rows.
struct JresPlan {
    bool on = false;
    int nb = 0, core = 0, K = 0, rounds = 0;
    bool half = false;  // half-height regions (jres_region_rows)
};

// The halo columns of a strip on each side: T, rounded up to the columns per lane so each lane's
// column vector (and the one vector store per lane) stays aligned.
inline int strip_halo(int T) { return (T + kJacobiCols - 1) / kJacobiCols * kJacobiCols; }

// Strips of a depth-T pass over a level w wide: 64 lanes of kJacobiCols columns, of which Tp on
// each side are halo and V are stored.
struct StripGeom {
    int Tp, V, nstrips;
};
inline StripGeom strip_geometry(int T, int w)
{
    const int Tp = strip_halo(T), V = 64 * kJacobiCols - 2 * Tp;
    return {Tp, V, (w + V - 1) / V};
}

int jacobi_tcap(const LevelDims& L);
// The streaming passes of a level (of band_rows of its rows; 0: the whole band).
std::vector<PassPlan> plan_level(pf_ctx* c, const LevelDims& L, int tcap, int batch, bool fast,
                                 int band_rows = 0);
// The row chunking of one depth-T band pass (one panorama) over band_rows rows.
PassPlan plan_band_pass(pf_ctx* c, const LevelDims& L, int T, int band_rows, bool fast);
JresPlan jres_plan(pf_ctx* c, const LevelDims& L, int batch, bool fast);

// ---- pf_fuse.hip ----------------------------------------------------------------------------
// SolveDepthAll for a batch on c->stream (pf_fuse's body after its checks); with c->wts set the
// targets are the weighted gather's.
int fuse_impl(pf_ctx* c, const float* emap, int ew, int eh, int ec, const float* tiles,
              const float* coeffs, int batch, int out_w, int out_h, float zr0, float zr1,
              uint16_t* out);
// What run_jacobi sweeps.  The first pass reads `first` (SRC_SEED 2: emap, SRC_UPSAMPLE 1: prev
// level, SRC_BUF 0: buffer a); passes ping-pong between a and b.  With out != nullptr the last
// pass stores the u16 quantisation instead of floats.  hcol: the level's packed-form certificate
// or nullptr; jp: the resident plan (nullptr or !on: streaming passes).
struct JacobiRun {
    int first;
    const float* emap;
    int ew, eh, ec;
    long long estride;
    const GridCol* cols;
    const GridRow* rows;
    const float* prev;
    long long pstride;
    const float* lnorm;
    float *a, *b;
    uint16_t* out;
    long long ostride;
    int batch;
    const float* hcol;
    const JresPlan* jp;
};

// Runs L.iters sweeps; returns the buffer holding the result (unused when out is given), or
// nullptr when a seeded run lacks its seed tables.
float* run_jacobi(pf_ctx* c, const LevelDims& L, const JacobiRun& r, int* npasses = nullptr);
// Under PF_JPLAN, the `jacobi plan ... sweeps` line of a level that takes the per-sweep form.
void show_sweeps_plan(const LevelDims& L, int batch);
// The JacobiPass fields that do not depend on the pass, over the whole band [h0, h1].
JacobiPass jacobi_pass(const pf_ctx* c, const LevelDims& L, const JacobiRun& r);
int seed_tables(pf_ctx* c, const LevelDims& L, int ew, int eh, int ec);
int jres_prepare(pf_ctx* c, const LevelDims& L, int batch, const JresPlan& jp);

// The strips and row chunks of one pass: depth T, band_rows rows in (at most) nchunks chunks.
inline void set_pass_shape(JacobiPass& P, int T, int band_rows, int nchunks)
{
    const StripGeom g = strip_geometry(T, P.w);
    P.Tp = g.Tp;
    P.V = g.V;
    P.nstrips = g.nstrips;
    P.rows_per_chunk = (band_rows + nchunks - 1) / nchunks;
    P.nchunks = (band_rows + P.rows_per_chunk - 1) / P.rows_per_chunk;
}

// Whether c->seed_ecol / seed_erow are the tables of this level and baseline size.
inline bool seed_tables_match(const pf_ctx* c, const LevelDims& L, int ew, int eh, int ec)
{
    const int key[5] = {L.w, L.h, ew, eh, ec};
    return memcmp(key, c->seed_key, sizeof(key)) == 0;
}

// ---- pf_ctx.hip -----------------------------------------------------------------------------
int jres_check(pf_ctx* c);
int ensure_err_host(pf_ctx* c);

}  // namespace pf
