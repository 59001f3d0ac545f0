// pf_fuse.hip -- the stream-ordered launch sequences of the fusion: the Jacobi driver, the
// levels of SolveDepthAll, and the drop-in entry points pf_register / pf_fuse / pf_merge.
#include "pf_ctx.hpp"

#include <cstdlib>

using namespace pf;

// SRC_SEED passes: ValueAtCoord's index (emap_index) split into its column term x * ec and row
// term y * ew * ec over the level's grid (the az / zen of grid_tables, then emap_index's fp64
// expression), cached per (level size, emap size).  Built by fuse_range before the level's
// timed Jacobi stage (the upload synchronises the stream); returns PF_OK or the upload's error.
int pf::seed_tables(pf_ctx* c, const LevelDims& L, int ew, int eh, int ec)
{
    if (seed_tables_match(c, L, ew, eh, ec)) return PF_OK;
    std::vector<int> ecol(L.w + 2), erow(L.h + 2);
    for (int xx = -1; xx <= L.w; xx++) {
        const float az = (float)((double)((float)xx / (float)(L.w - 1) * 2.0f) * PF_MYPI);
        ecol[xx + 1] = (int)((double)az / (PF_MYPI * 2) * (double)(float)(ew - 1)) * ec;
    }
    for (int yy = -1; yy <= L.h; yy++) {
        const float zen = (float)((double)((float)yy / (float)(L.h - 1)) * PF_MYPI);
        erow[yy + 1] = (int)((double)zen / PF_MYPI * (double)(float)(eh - 1)) * ew * ec;
    }
    int rc;
    if ((rc = upload(c, c->seed_ecol, ecol)) || (rc = upload(c, c->seed_erow, erow))) return rc;
    const int key[5] = {L.w, L.h, ew, eh, ec};
    memcpy(c->seed_key, key, sizeof(key));
    return PF_OK;
}

// The resident kernel's buffers (outside the timed stage: a first allocation synchronises).
int pf::jres_prepare(pf_ctx* c, const LevelDims& L, int batch, const JresPlan& jp)
{
    int rc;
    // hand-off rows [batch][nb][2 parity][2 edge][K][w] (JresArgs::xbuf)
    const size_t xb = sizeof(float) * (size_t)batch * jp.nb * 4 * (size_t)jp.K * L.w;
    if ((rc = ensure(c, c->jres_x, xb))) return rc;
    // ticket, error count, one flag word per row block
    const size_t sb = sizeof(uint32_t) * (2 + (size_t)batch * jp.nb);
    if ((rc = ensure_err_host(c))) return rc;
    if (c->jres_sync.bytes < sb) {
        if ((rc = ensure(c, c->jres_sync, sb))) return rc;
        HIPCHK(c, hipMemsetAsync(c->jres_sync.p, 0, sb, c->stream));
        c->jres_tk = 0;
        c->jres_fb = 1;
    }
    return PF_OK;
}

JacobiPass pf::jacobi_pass(const pf_ctx* c, const LevelDims& L, const JacobiRun& r)
{
    const long long st = (long long)L.w * L.h;
    JacobiPass P{};
    if (r.first == 2 && r.emap) {  // the tables seed_tables() built for this level and emap
        P.ecol = (const int*)c->seed_ecol.p;
        P.erow = (const int*)c->seed_erow.p;
    }
    P.prev = r.prev; P.pstride = r.pstride;
    P.emap = r.emap; P.estride = r.estride; P.ew = r.ew; P.eh = r.eh; P.ec = r.ec;
    P.cols = r.cols; P.rows = r.rows;
    P.lnorm = r.lnorm; P.lstride = st;
    P.sstride = st; P.dstride = st;
    P.out = r.out; P.ostride = r.ostride;
    P.w = L.w; P.h = L.h; P.h0 = L.h0; P.h1 = L.h1;
    P.hcol = r.hcol;
    P.row_lo = L.h0;
    P.row_hi = L.h1 + 1;
    return P;
}

static bool show_plans()
{
    static const bool show = getenv("PF_JPLAN") != nullptr;
    return show;
}

// The per-sweep form's line among the PF_JPLAN lines (run_jres and run_jacobi print the others).
void pf::show_sweeps_plan(const LevelDims& L, int batch)
{
    if (show_plans())
        fprintf(stderr, "jacobi plan %dx%d band %d iters %d batch %d sweeps\n", L.w, L.h,
                L.h1 - L.h0 + 1, L.iters, batch);
}

// All of a level's sweeps in one launch of the resident kernel (pf_jres.hip).
static float* run_jres(pf_ctx* c, const LevelDims& L, const JacobiRun& r, const JresPlan& jp)
{
    JresArgs A{};
    A.src_mode = r.first;
    if (r.first == 2) {
        if (!r.emap || !seed_tables_match(c, L, r.ew, r.eh, r.ec)) return nullptr;
        A.ecol = (const int*)c->seed_ecol.p;
        A.erow = (const int*)c->seed_erow.p;
    }
    const long long st = (long long)L.w * L.h;
    A.src = r.a; A.sstride = st;
    A.prev = r.prev; A.pstride = r.pstride;
    A.emap = r.emap; A.estride = r.estride;
    A.lnorm = r.lnorm; A.lstride = st;
    A.hcol = r.hcol;
    float* dst = r.first == 0 ? r.b : r.a;
    A.dst = dst; A.dstride = st;
    A.out = r.out; A.ostride = r.ostride;
    A.w = L.w; A.h = L.h; A.h0 = L.h0; A.h1 = L.h1; A.iters = L.iters; A.batch = r.batch;
    A.nb = jp.nb; A.core = jp.core; A.K = jp.K; A.half = jp.half ? 1 : 0;
    uint32_t* sync = (uint32_t*)c->jres_sync.p;
    A.xbuf = (float*)c->jres_x.p;
    A.ticket = sync;
    A.err = sync + 1;
    A.flags = sync + 2;
    A.err_host = c->jres_err_h;  // mapped + coherent: the device pointer is the host one
    static const int dbg = getenv("PF_JRES_DBG") ? atoi(getenv("PF_JRES_DBG")) : 0;
    A.dbg = dbg;
    A.spin_log2 = 24;
    if (c->jres_fault) {  // pf_debug_jres_fault: this launch only
        A.dbg |= 16;
        A.spin_log2 = c->jres_fault;
        c->jres_fault = 0;
    }
    A.tbase = c->jres_tk;
    A.fbase = c->jres_fb;
    c->jres_tk += (uint32_t)(r.batch * jp.nb);
    c->jres_fb += (uint32_t)(jp.rounds + 1);
    if (show_plans())
        fprintf(stderr, "jacobi plan %dx%d band %d iters %d batch %d resident: nb %d core %d K %d rounds %d\n",
                L.w, L.h, L.h1 - L.h0 + 1, L.iters, r.batch, jp.nb, jp.core, jp.K, jp.rounds);
    launch_jres(c->stream, A);
    // the error word, stream-ordered into pinned memory: jres_check reports it
    return dst;
}

float* pf::run_jacobi(pf_ctx* c, const LevelDims& L, const JacobiRun& r, int* npasses)
{
    if (r.jp && r.jp->on) {
        if (npasses) *npasses = 1;
        return run_jres(c, L, r, *r.jp);
    }
    static const bool slow = getenv("PF_JSLOW") != nullptr;  // force the general (scalar) form
    // packed form: the level's separable-coverage certificate (pf_jacobi.hip)
    const bool fast = r.hcol && !slow;
    const std::vector<PassPlan> plan = plan_level(c, L, jacobi_tcap(L), r.batch, fast);
    if (r.first == 2 && r.emap && !seed_tables_match(c, L, r.ew, r.eh, r.ec)) return nullptr;
    JacobiPass P = jacobi_pass(c, L, r);
    const int band_rows = L.h1 - L.h0 + 1;
    float* src = (r.first == 0) ? r.a : nullptr;
    float* dst = (r.first == 0) ? r.b : r.a;
    if (show_plans()) {
        fprintf(stderr, "jacobi plan %dx%d band %d iters %d batch %d %s C%d:", L.w, L.h,
                band_rows, L.iters, r.batch, fast ? "packed" : "general", kJacobiCols);
        for (const PassPlan& pp : plan)
            fprintf(stderr, " T%d/n%d%s", pp.T, pp.nchunks, pp.stages > 1 ? "p" : "");
        fprintf(stderr, "\n");
    }
    int pass = 0;
    for (const PassPlan& pp : plan) {
        const int T = pp.T;
        set_pass_shape(P, T, band_rows, pp.nchunks);
        P.src_mode = pass == 0 ? r.first : 0;
        P.src = src;
        P.dst = dst;
        P.out_mode = (pass + 1 == (int)plan.size() && r.out) ? 1 : 0;
        if (pp.stages > 1) launch_jpipe(c->stream, P, pp.stages, T / pp.stages, r.batch);
        else launch_jstream(c->stream, P, T, r.batch, fast);
        src = dst;
        dst = (dst == r.a) ? r.b : r.a;
        pass++;
    }
    if (npasses) *npasses = pass;
    return src;
}

// PF_WTGT_LEVELS=1 (read per call): the weighted fusion gathers its targets level by level
// (k_targets_patch_weighted) instead of in one launch; the planes are the same bit for bit.
static bool weighted_per_level()
{
    const char* e = getenv("PF_WTGT_LEVELS");
    return e && e[0] == '1';
}

// Floats of the per-level target planes of one panorama (fuse_range's lnorm workspace).
static long long target_planes(const LevelCache& lc)
{
    long long n = 0;
    for (int l = 0; l < lc.nlevels; l++) n += (long long)lc.dims[l].w * lc.dims[l].h;
    return n;
}

// The fusion levels of panoramas [0, batch) of the given pointers, on c->stream.  ws are the
// level-buffer bases (pano b of a level with stride st at base + b*st); lnorm_ws holds one target
// plane per level (level l at lnorm_ws + batch * sum_{k<l} st_k), target_planes() * batch floats.
//
// The target planes depend only on the tiles and the coefficients, not on any Jacobi result, so
// every level's plane is gathered first, in one launch (k_targets_multi).
static int fuse_range(pf_ctx* c, const float* emap, int ew, int eh, int ec, const float* tiles,
                      const float* coeffs, int batch, int out_w, int out_h, uint16_t* out,
                      float* const ws[3], float* lnorm_ws)
{
    const long long plane = (long long)out_w * out_h;
    const long long estride = (long long)ew * eh * ec;
    float* bufs[3] = {ws[0], ws[1], ws[2]};
    float* prev = nullptr;
    LevelCache& lc = c->lc;
    // PF_JACOBI=naive: one launch per sweep (the form a level with jacobi_tcap(L) < 1 runs)
    static const bool naive = getenv("PF_JACOBI") && strcmp(getenv("PF_JACOBI"), "naive") == 0;
    float* lnl[4] = {};
    {
        long long off = 0;
        for (int l = 0; l < lc.nlevels; l++) {
            lnl[l] = lnorm_ws + off;
            off += (long long)lc.dims[l].w * lc.dims[l].h * batch;
        }
    }
    {
        TgtMulti M{};
        M.nlev = lc.nlevels;
        M.nentries = lc.tgt_nentries;
        const int pw_ = targets_patch_w(), ph_ = targets_patch_h();
        double bytes = 0;
        for (int l = 0; l < lc.nlevels; l++) {
            const LevelDims& L = lc.dims[l];
            TgtLevel& T = M.lv[l];
            T.tmask = (const uint32_t*)lc.tmask[l].p;
            T.nmw = (c->ntiles + 31) / 32;
            T.L = L;
            T.box = (const TileBox*)lc.box[l].p;
            T.tb = (const TapBox*)lc.tapbox[l].p;
            T.map = (const int32_t*)lc.tapmap[l].p;
            T.lnorm = lnl[l];
            T.lstride = (long long)L.w * L.h;
            T.npx = (L.w + pw_ - 1) / pw_;
            T.npy = (L.h1 - L.h0 + 1 + ph_ - 1) / ph_;
            bytes += (double)batch * (4.0 * L.w * (L.h1 - L.h0 + 1) + 4.0 * (double)lc.taps[l]);
        }
        StageTimer t(c, PF_STAGE_TARGETS, bytes, 1);
        if (c->wts && weighted_per_level()) {  // pf_fuse_weighted, one launch per level
            t.set_launches(lc.nlevels);
            for (int l = 0; l < lc.nlevels; l++) {
                const TgtLevel& T = M.lv[l];
                launch_targets_patch_weighted(c->stream, (const TileGeom*)c->geom.p, T.box, T.tb,
                                              c->ntiles, T.map, tiles, c->tile_elems, c->wts,
                                              c->wts_stride, coeffs, T.L, T.lnorm, T.lstride,
                                              batch, T.tmask, T.nmw);
            }
        } else if (c->wts) {  // pf_fuse_weighted / pf_merge_weighted
            launch_targets_multi_weighted(c->stream, (const TileGeom*)c->geom.p, c->ntiles, tiles,
                                          c->tile_elems, c->wts, c->wts_stride, coeffs, M,
                                          (const int2*)lc.tgt_order.p, batch);
        } else {
            launch_targets_multi(c->stream, (const TileGeom*)c->geom.p, c->ntiles, tiles,
                                 c->tile_elems, coeffs, M, (const int2*)lc.tgt_order.p, batch,
                                 c->valid);
        }
    }
    for (int l = 0; l < lc.nlevels; l++) {
        const LevelDims& L = lc.dims[l];
        const long long st = (long long)L.w * L.h;
        const bool last = l == lc.nlevels - 1;
        const long long pst = l > 0 ? (long long)lc.dims[l - 1].w * lc.dims[l - 1].h : 0;
        float* a = nullptr;
        float* b = nullptr;
        for (int k = 0; k < 3; k++) {
            if (bufs[k] == prev) continue;
            if (!a) a = bufs[k];
            else if (!b) b = bufs[k];
        }
        const double B = (double)batch;
        const double band = (double)L.w * (L.h1 - L.h0 + 1);
        const GridCol* cols = (const GridCol*)lc.cols[l].p;
        const GridRow* rows = (const GridRow*)lc.rows[l].p;
        float* const lnorm_l = lnl[l];
        float* res = nullptr;
        if (naive || jacobi_tcap(L) < 1) {
            show_sweeps_plan(L, batch);
            {
                double srcb = l == 0 ? band * 4.0 : (double)st;
                StageTimer t(c, PF_STAGE_SEED, B * (4.0 * st + srcb), 1);
                if (l == 0)
                    launch_seed0(c->stream, emap, ew, eh, ec, estride, cols, rows, L, a, st, batch);
                else
                    launch_upsample(c->stream, prev, pst, L, a, st, batch);
            }
            HIPCHK(c, hipMemcpyAsync(b, a, sizeof(float) * st * batch, hipMemcpyDeviceToDevice,
                                     c->stream));
            {
                StageTimer t(c, PF_STAGE_JACOBI, B * 12.0 * band * L.iters, L.iters);
                launch_jacobi(c->stream, a, b, (const float*)lnorm_l, st, L, L.iters, batch,
                              &res);
            }
            if (last) {
                StageTimer t(c, PF_STAGE_QUANTIZE, B * 6.0 * st, 1);
                launch_quantize(c->stream, res, st, (int)st, out, plane, batch);
            }
        } else {
            {
                // out-of-band rows: zero / upsampled copy (u16 on the last level)
                double nb = (double)st - band;
                StageTimer t(c, PF_STAGE_SEED, B * nb * (last ? 3.0 : 9.0), 1);
                launch_border(c->stream, l == 0 ? nullptr : prev, pst, L, a, b, st,
                              last ? out : nullptr, plane, batch);
            }
            if (l == 0) {  // outside the timed stage: the first call per emap size uploads
                int rc;
                if ((rc = seed_tables(c, L, ew, eh, ec))) return rc;
            }
            const JresPlan jp = jres_plan(c, L, batch, level_full(c, l));
            if (jp.on) {  // outside the timed stage too (first allocation synchronises)
                int rc;
                if ((rc = jres_prepare(c, L, batch, jp))) return rc;
            }
            {
                // 12 B per pixel-update (read b, read L, write b'), SURVEY.md 8d
                StageTimer t(c, PF_STAGE_JACOBI, B * 12.0 * band * L.iters, L.iters);
                int passes = 0;
                JacobiRun r{};
                r.first = l == 0 ? 2 : 1;
                r.emap = emap; r.ew = ew; r.eh = eh; r.ec = ec; r.estride = estride;
                r.cols = cols; r.rows = rows;
                r.prev = prev; r.pstride = pst;
                r.lnorm = lnorm_l; r.a = a; r.b = b;
                r.out = last ? out : nullptr; r.ostride = plane;
                r.batch = batch;
                r.hcol = level_full(c, l) ? (const float*)lc.hcol[l].p : nullptr;
                r.jp = &jp;
                res = run_jacobi(c, L, r, &passes);
                t.set_launches(passes);  // k_jlag launches (rocprof's count for that kernel)
            }
            if (!res) return fail(c, PF_EINVAL, "level-0 seed tables missing");
        }
        prev = res;
        if (!c->ev_level[l]) HIPCHK(c, hipEventCreateWithFlags(&c->ev_level[l], hipEventDisableTiming));
        HIPCHK(c, hipEventRecord(c->ev_level[l], c->stream));
    }
    c->nlev_recorded = lc.nlevels;
    HIPCHK(c, hipGetLastError());
    return PF_OK;
}

// SolveDepthAll for a batch, on c->stream.  (Running the batch as two staggered halves on two
// streams, so that one half's coarse levels overlap the other's fine levels, was measured slower:
// 10.4-10.6k vs 11.6k panoramas/s at batch 64 -- the half-size passes lose more than the
// overlap wins.)
int pf::fuse_impl(pf_ctx* c, const float* emap, int ew, int eh, int ec, const float* tiles,
                  const float* coeffs, int batch, int out_w, int out_h, float zr0, float zr1,
                  uint16_t* out)
{
    int rc;
    if ((rc = prepare_levels(c, out_w, out_h, zr0, zr1))) return rc;
    const long long plane = (long long)out_w * out_h;
    for (int k = 0; k < 3; k++)
        if ((rc = ensure(c, c->buf[k], sizeof(float) * plane * batch))) return rc;
    if ((rc = ensure(c, c->lnorm, sizeof(float) * target_planes(c->lc) * batch))) return rc;
    float* ws[3] = {(float*)c->buf[0].p, (float*)c->buf[1].p, (float*)c->buf[2].p};
    return fuse_range(c, emap, ew, eh, ec, tiles, coeffs, batch, out_w, out_h, out, ws,
                      (float*)c->lnorm.p);
}

// pf_register / pf_register_ex.  The launchers branch on the context's loss and tile depth:
// without either this launches what pf_register always did.  apply_dst (planar tiles only, with
// apply): where the transformed tiles go; nullptr: in place.
static int register_impl(pf_ctx* c, const float* emap, int ew, int eh, int ec, float* tiles,
                         int batch, float zr0, float zr1, int degree, int apply, float* coeffs,
                         double* coeffs64, double* summary, float* apply_dst = nullptr)
{
    int rc;
    if ((rc = check_common(c, batch))) return rc;
    if ((rc = check_emap(c, emap, ew, eh, ec))) return rc;
    if (!tiles) return fail(c, PF_EINVAL, "tiles is NULL");
    if (degree < 0 || degree > 3) return fail(c, PF_EINVAL, "degree %d not in [0,3]", degree);
    const bool robust = c->loss_kind != PF_LOSS_NONE;
    if (summary && !robust)
        return fail(c, PF_EINVAL,
                    "pf_register_ex: summary needs a loss (pf_set_register_loss); the moment-sum "
                    "solve has none to report");
    if (robust && (degree != 3 || c->solver != PF_SOLVER_LM))
        return fail(c, PF_EINVAL,
                    "the loss of pf_set_register_loss needs degree 3 and PF_SOLVER_LM (got degree "
                    "%d, solver %d)",
                    degree, c->solver);
    if ((rc = prepare_registration(c, zr0, zr1))) return rc;
    if ((rc = check_reg_grids(c, nullptr))) return rc;
    float* cf = coeffs;
    if (!cf) {
        if ((rc = ensure(c, c->coeffs, sizeof(float) * 4 * c->ntiles * batch))) return rc;
        cf = (float*)c->coeffs.p;
    }
    double nsamp = 0;
    for (const RegGrid& g : c->reg_h) nsamp += (double)(g.cols + 1) * (g.rows + 1);
    const int2* sidx = reg_sample_index(c, ew, eh, ec);  // before the stage timer: built once
    if (robust && !sidx) return fail(c, PF_EHIP, "robust registration: no sample-index table");
    const bool planar = c->tile_depth == PF_TILE_DEPTH_PLANAR;
    const float* kfs = planar ? reg_sample_kf(c, ew, eh, ec) : nullptr;
    if (planar && !kfs) return fail(c, PF_EHIP, "planar registration: no sample ray-factor table");
    if (planar) {
        const TileGeom* geom = (const TileGeom*)c->geom.p;
        const RegGrid* reg = (const RegGrid*)c->reg.p;
        const long long estride = (long long)ew * eh * ec;
        StageTimer t(c, PF_STAGE_REGISTER,
                     batch * (12.0 * nsamp + (apply ? 8.0 * (double)c->tile_elems / c->tile_c : 0.0)),
                     apply ? 2 : 1);
        if (robust)
            launch_register_robust_planar(c->stream, geom, reg, c->ntiles, emap, estride, tiles,
                                          c->tile_elems, sidx, kfs, cf, coeffs64, summary, batch,
                                          c->loss_kind, c->loss_a, c->valid);
        else
            launch_register_planar(c->stream, geom, reg, c->ntiles, emap, estride, tiles,
                                   c->tile_elems, degree, c->solver, cf, coeffs64, batch, sidx, kfs,
                                   c->valid);
        if (apply)
            launch_apply_cubic_planar(c->stream, geom, (const RayTile*)c->ray.p,
                                      (const double*)c->ray_tab.p, c->ntiles,
                                      c->tile_elems / c->tile_c, tiles,
                                      apply_dst ? apply_dst : tiles, c->tile_elems, cf, batch,
                                      c->valid);
    } else {
        StageTimer t(c, PF_STAGE_REGISTER,
                     batch * (8.0 * nsamp + (apply ? 8.0 * (double)c->tile_elems / c->tile_c : 0.0)),
                     apply ? 2 : 1);
        if (robust)
            launch_register_robust(c->stream, (const TileGeom*)c->geom.p, (const RegGrid*)c->reg.p,
                                   c->ntiles, emap, (long long)ew * eh * ec, tiles, c->tile_elems,
                                   sidx, cf, coeffs64, summary, batch, c->loss_kind, c->loss_a,
                                   c->valid);
        else
            launch_register(c->stream, (const TileGeom*)c->geom.p, (const RegGrid*)c->reg.p,
                            (const GridCol*)c->rcols.p, (const GridRow*)c->rrows.p, c->ntiles,
                            emap, ew, eh, ec, (long long)ew * eh * ec, tiles, c->tile_elems,
                            degree, c->solver, cf, coeffs64, batch, nullptr, nullptr, sidx,
                            c->valid);
        if (apply)
            launch_apply_cubic(c->stream, (const TileGeom*)c->geom.p, c->ntiles,
                               c->tile_elems / c->tile_c, tiles, c->tile_elems, cf, batch,
                               c->valid);
    }
    HIPCHK(c, hipGetLastError());
    return PF_OK;
}

extern "C" {

int pf_register(pf_ctx* c, const float* emap, int ew, int eh, int ec, float* tiles, int batch,
                float zr0, float zr1, int degree, int apply, float* coeffs, double* coeffs64)
{
    return register_impl(c, emap, ew, eh, ec, tiles, batch, zr0, zr1, degree, apply, coeffs,
                         coeffs64, nullptr);
}

int pf_register_ex(pf_ctx* c, const float* emap, int ew, int eh, int ec, float* tiles, int batch,
                   float zr0, float zr1, int degree, int apply, float* coeffs, double* coeffs64,
                   double* summary)
{
    return register_impl(c, emap, ew, eh, ec, tiles, batch, zr0, zr1, degree, apply, coeffs,
                         coeffs64, summary);
}

int pf_set_register_loss(pf_ctx* c, int kind, double a)
{
    if (!c) return PF_EINVAL;
    if (kind != PF_LOSS_NONE && kind != PF_LOSS_HUBER && kind != PF_LOSS_SOFTL1)
        return fail(c, PF_EINVAL, "pf_set_register_loss: unknown loss %d", kind);
    if (kind != PF_LOSS_NONE && !(std::isfinite(a) && a > 0.0))
        return fail(c, PF_EINVAL, "pf_set_register_loss: needs a finite scale a > 0 (got %g)", a);
    c->loss_kind = kind;
    c->loss_a = kind == PF_LOSS_NONE ? 0.0 : a;
    return PF_OK;
}

int pf_fuse(pf_ctx* c, const float* emap, int ew, int eh, int ec, const float* tiles,
            const float* coeffs, int batch, int out_w, int out_h, float zr0, float zr1,
            uint16_t* out)
{
    int rc;
    if ((rc = check_common(c, batch))) return rc;
    if ((rc = check_emap(c, emap, ew, eh, ec))) return rc;
    if (!tiles || !out) return fail(c, PF_EINVAL, "tiles/out is NULL");
    if ((rc = check_ray_coeffs(c, "pf_fuse", coeffs))) return rc;
    if ((rc = jres_check(c))) return rc;  // an earlier fusion's timeout, once it has landed
    return fuse_impl(c, emap, ew, eh, ec, tiles, coeffs, batch, out_w, out_h, zr0, zr1, out);
}

int pf_merge(pf_ctx* c, const float* emap, int ew, int eh, int ec, const float* tiles, int batch,
             int out_w, float zr0, float zr1, float* coeffs, uint16_t* out)
{
    int rc;
    if ((rc = check_common(c, batch))) return rc;
    if ((rc = check_emap(c, emap, ew, eh, ec))) return rc;
    if (!tiles || !out) return fail(c, PF_EINVAL, "tiles/out is NULL");
    if ((rc = jres_check(c))) return rc;  // an earlier fusion's timeout, once it has landed
    float* cf = coeffs;
    if (!cf) {
        if ((rc = ensure(c, c->coeffs, sizeof(float) * 4 * c->ntiles * batch))) return rc;
        cf = (float*)c->coeffs.p;
    }
    if (c->tile_depth == PF_TILE_DEPTH_PLANAR) {
        // planar-depth tiles: the fused-transform gather has no ray factor, so the planar fit is
        // applied into a copy of the tiles, which is fused without coefficients.  Its invalid
        // pixels are the NaNs apply wrote: the copy is fused under (-inf, +inf), not under the
        // caller's lo / hi (a value clamped to exactly 0 is valid).
        if ((rc = ensure(c, c->disp_tiles, sizeof(float) * (size_t)c->tile_elems * batch)))
            return rc;
        float* copy = (float*)c->disp_tiles.p;
        if ((rc = register_impl(c, emap, ew, eh, ec, const_cast<float*>(tiles), batch, zr0, zr1, 3,
                                1, cf, nullptr, nullptr, copy)))
            return rc;
        const TileValid rule = c->valid;
        if (rule.on) c->valid = TileValid{1, -INFINITY, INFINITY};
        rc = fuse_impl(c, emap, ew, eh, ec, copy, nullptr, batch, out_w, out_w / 2, zr0, zr1, out);
        c->valid = rule;
        return rc;
    }
    if ((rc = pf_register(c, emap, ew, eh, ec, const_cast<float*>(tiles), batch, zr0, zr1, 3, 0,
                          cf, nullptr)))
        return rc;
    return fuse_impl(c, emap, ew, eh, ec, tiles, cf, batch, out_w, out_w / 2, zr0, zr1, out);
}

int pf_register_joint(pf_ctx* c, const float* emap, int ew, int eh, int ec, const float* tiles,
                      int batch, float zr0, float zr1, int degree, const int* active,
                      float* coeffs, double* coeffs64)
{
    int rc;
    if ((rc = check_common(c, batch))) return rc;
    if ((rc = check_no_loss(c, "pf_register_joint"))) return rc;
    if (c->tile_depth != PF_TILE_DEPTH_RAY)
        return fail(c, PF_ESTATE,
                    "pf_register_joint has no planar-depth form: call pf_set_tile_depth(ctx, "
                    "PF_TILE_DEPTH_RAY) first");
    if ((rc = check_emap(c, emap, ew, eh, ec))) return rc;
    if (!tiles || !active) return fail(c, PF_EINVAL, "tiles/active is NULL");
    if (degree < 0 || degree > 3) return fail(c, PF_EINVAL, "degree %d not in [0,3]", degree);
    if ((rc = prepare_registration(c, zr0, zr1))) return rc;
    std::vector<int> act(active, active + c->ntiles);
    int nact = 0;
    for (int v : act) nact += v != 0;
    if (nact == 0) return fail(c, PF_EINVAL, "pf_register_joint: no active tile");
    if ((rc = check_reg_grids(c, act.data()))) return rc;
    if ((rc = upload(c, c->reg_active, act))) return rc;
    if ((rc = ensure(c, c->reg_sums,
                     sizeof(double) * register_sums_per_tile() * c->ntiles * batch)))
        return rc;
    float* cf = coeffs;
    if (!cf) {
        if ((rc = ensure(c, c->coeffs, sizeof(float) * 4 * batch))) return rc;
        cf = (float*)c->coeffs.p;
    }
    launch_register(c->stream, (const TileGeom*)c->geom.p, (const RegGrid*)c->reg.p,
                    (const GridCol*)c->rcols.p, (const GridRow*)c->rrows.p, c->ntiles, emap, ew,
                    eh, ec, (long long)ew * eh * ec, tiles, c->tile_elems, degree, c->solver,
                    nullptr, nullptr, batch, (double*)c->reg_sums.p,
                    (const int*)c->reg_active.p, reg_sample_index(c, ew, eh, ec), c->valid);
    launch_register_joint(c->stream, (const double*)c->reg_sums.p, (const int*)c->reg_active.p,
                          c->ntiles, batch, degree, c->solver, cf, coeffs64, c->valid.on != 0);
    HIPCHK(c, hipGetLastError());
    return PF_OK;
}

int pf_set_tile_validity(pf_ctx* c, int mode, float lo, float hi)
{
    if (!c) return PF_EINVAL;
    if (mode != PF_VALID_ALL && mode != PF_VALID_RANGE)
        return fail(c, PF_EINVAL, "pf_set_tile_validity: unknown mode %d", mode);
    if (mode == PF_VALID_RANGE && !(lo < hi))
        return fail(c, PF_EINVAL, "pf_set_tile_validity: needs lo < hi (got %g, %g)", (double)lo,
                    (double)hi);
    c->valid.on = mode == PF_VALID_RANGE ? 1 : 0;
    c->valid.lo = c->valid.on ? lo : 0.0f;
    c->valid.hi = c->valid.on ? hi : 0.0f;
    return PF_OK;
}

int pf_tile_valid_counts(pf_ctx* c, const float* tiles, const float* emap, int ew, int eh, int ec,
                         int batch, float zr0, float zr1, long long* counts)
{
    int rc;
    if ((rc = check_common(c, batch))) return rc;
    if ((rc = check_emap(c, emap, ew, eh, ec))) return rc;
    if (!tiles || !counts) return fail(c, PF_EINVAL, "tiles/counts is NULL");
    if ((rc = prepare_registration(c, zr0, zr1))) return rc;
    if ((rc = check_reg_grids(c, nullptr))) return rc;
    const int2* sidx = reg_sample_index(c, ew, eh, ec);
    if (!sidx) return fail(c, PF_ENOMEM, "pf_tile_valid_counts: no registration sample index");
    launch_valid_counts(c->stream, (const TileGeom*)c->geom.p, (const RegGrid*)c->reg.p, c->ntiles,
                        emap, (long long)ew * eh * ec, tiles, c->tile_elems, sidx, c->valid,
                        counts, batch);
    HIPCHK(c, hipGetLastError());
    return PF_OK;
}

}  // extern "C"
