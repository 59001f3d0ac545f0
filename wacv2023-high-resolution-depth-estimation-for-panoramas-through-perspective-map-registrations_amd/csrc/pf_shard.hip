// pf_shard.hip -- the level-by-level entry points of the sharded fusion (pf_dist): tile-range
// partial sums, row-restricted pieces, whole levels from summed targets and single band passes.
// Each opens with check_common, its NULL checks and level_at (pf_ctx.hpp), in the order its
// callers have come to see the errors in.
#include "pf_ctx.hpp"

#include <algorithm>

using namespace pf;

// The level's packed-form certificate (LevelCache::hcol), or nullptr where it has none.
static const float* level_hcol(const pf_ctx* c, int level)
{
    return level_full(c, level) ? (const float*)c->lc.hcol[level].p : nullptr;
}

// The sweeps' result `res` back into `buf`: its band rows (the other rows of the two are equal).
static int band_back(pf_ctx* c, const LevelDims& L, float* buf, const float* res)
{
    const int ba = std::max(L.h0, 0), bb = std::min(L.h1 + 1, L.h);  // band rows [ba, bb)
    if (res != buf && bb > ba)
        HIPCHK(c, hipMemcpyAsync(buf + (size_t)ba * L.w, res + (size_t)ba * L.w,
                                 sizeof(float) * (size_t)L.w * (bb - ba),
                                 hipMemcpyDeviceToDevice, c->stream));
    return PF_OK;
}

// Row-restricted pieces of the sharded fusion (pf_dist.fuse_row_sharded): a rank computes only
// the rows it sweeps (plus halo) and the rows its tiles send to its neighbours.
static int level_rows(pf_ctx* c, int out_w, int out_h, float zr0, float zr1, int level, int& row0,
                      int& row1, const LevelDims** L)
{
    int rc;
    if ((rc = check_common(c, 1))) return rc;
    if ((rc = level_at(c, out_w, out_h, zr0, zr1, level, L))) return rc;
    if (row0 < 0 || row1 > (*L)->h || row0 > row1)
        return fail(c, PF_EINVAL, "rows [%d,%d) outside [0,%d)", row0, row1, (*L)->h);
    // rows of the range outside the band [h0, h1] are written too: no targets there (zero sums and
    // counts, the un-windowed marker), as in the whole-plane calls
    return PF_OK;
}

static int targets_partial(pf_ctx* c, const float* tiles, const float* coeffs, int t0, int t1,
                           int level, const LevelDims& L, float* lsum, float* cnt, int row0,
                           int row1)
{
    const LevelCache& lc = c->lc;
    HIPCHK(c, launch_targets_partial(c->stream, (const TileGeom*)c->geom.p,
                               (const TileBox*)lc.box[level].p, (const TapBox*)lc.tapbox[level].p,
                               (const uint32_t*)lc.tmask[level].p, (c->ntiles + 31) / 32, t0, t1,
                               (const int32_t*)lc.tapmap[level].p, tiles, coeffs, L, lsum, cnt,
                               row0, row1));
    HIPCHK(c, hipGetLastError());
    return PF_OK;
}

extern "C" {

int pf_fuse_partial(pf_ctx* c, const float* tiles, const float* coeffs, int t0, int t1,
                    int out_w, int out_h, float zr0, float zr1, int level, float* lsum,
                    float* cnt)
{
    int rc;
    const LevelDims* L = nullptr;
    if ((rc = check_common(c, 1))) return rc;
    if ((rc = check_unmasked(c, "pf_fuse_partial"))) return rc;
    if ((rc = check_ray_coeffs(c, "pf_fuse_partial", coeffs))) return rc;
    if (!tiles || !lsum || !cnt) return fail(c, PF_EINVAL, "NULL buffer");
    if ((rc = check_tile_range(c, t0, t1))) return rc;
    if ((rc = level_at(c, out_w, out_h, zr0, zr1, level, &L))) return rc;
    HIPCHK(c, hipMemsetAsync(lsum, 0, sizeof(float) * L->w * L->h, c->stream));
    HIPCHK(c, hipMemsetAsync(cnt, 0, sizeof(float) * L->w * L->h, c->stream));
    return targets_partial(c, tiles, coeffs, t0, t1, level, *L, lsum, cnt, L->h0, L->h1 + 1);
}

int pf_fuse_partial_rows(pf_ctx* c, const float* tiles, const float* coeffs, int t0, int t1,
                         int out_w, int out_h, float zr0, float zr1, int level, int row0,
                         int row1, float* lsum, float* cnt)
{
    int rc;
    const LevelDims* L = nullptr;
    if ((rc = check_unmasked(c, "pf_fuse_partial_rows"))) return rc;
    if ((rc = check_ray_coeffs(c, "pf_fuse_partial_rows", coeffs))) return rc;
    if ((rc = level_rows(c, out_w, out_h, zr0, zr1, level, row0, row1, &L))) return rc;
    if (!tiles || !lsum || !cnt) return fail(c, PF_EINVAL, "NULL buffer");
    if ((rc = check_tile_range(c, t0, t1))) return rc;
    return targets_partial(c, tiles, coeffs, t0, t1, level, *L, lsum, cnt, row0,
                           std::max(row0, row1));
}

int pf_fuse_coverage_rows(pf_ctx* c, int out_w, int out_h, float zr0, float zr1, int level,
                          int row0, int row1, float* cnt)
{
    int rc;
    const LevelDims* L = nullptr;
    if ((rc = check_unmasked(c, "pf_fuse_coverage_rows"))) return rc;
    if ((rc = level_rows(c, out_w, out_h, zr0, zr1, level, row0, row1, &L))) return rc;
    if (!cnt) return fail(c, PF_EINVAL, "NULL buffer");
    launch_coverage_rows(c->stream, (const TileBox*)c->lc.box[level].p, c->ntiles, *L, cnt, row0,
                         row1);
    HIPCHK(c, hipGetLastError());
    return PF_OK;
}

int pf_fuse_normalize_rows(pf_ctx* c, const float* lsum, const float* cnt, int out_w, int out_h,
                           float zr0, float zr1, int level, int row0, int row1, float* lnorm)
{
    int rc;
    const LevelDims* L = nullptr;
    if ((rc = level_rows(c, out_w, out_h, zr0, zr1, level, row0, row1, &L))) return rc;
    if (!lsum || !cnt || !lnorm) return fail(c, PF_EINVAL, "NULL buffer");
    if (row1 > row0) launch_normalize(c->stream, lsum, cnt, *L, lnorm, row0, row1);
    HIPCHK(c, hipGetLastError());
    return PF_OK;
}

int pf_fuse_tile_rows(pf_ctx* c, int out_w, int out_h, float zr0, float zr1, int level, int t0,
                      int t1, int* ymin, int* ymax)
{
    int rc;
    const LevelDims* L = nullptr;
    if ((rc = check_common(c, 1))) return rc;
    if (!ymin || !ymax) return fail(c, PF_EINVAL, "NULL output");
    if ((rc = level_at(c, out_w, out_h, zr0, zr1, level, &L))) return rc;
    if ((rc = check_tile_range(c, t0, t1))) return rc;
    int lo = INT32_MAX, hi = INT32_MIN;
    for (int p = t0; p < t1; p++) {  // rows where k_targets_patch_partial can write a non-zero sum
        const TileBox& b = c->lc.box_h[level][p];
        const int a = std::max(std::min(b.y0, b.y1), L->h0 + 1);
        const int z = std::min(std::max(b.y0, b.y1), L->h1 - 1);
        if (a > z) continue;
        lo = std::min(lo, a);
        hi = std::max(hi, z);
    }
    *ymin = lo == INT32_MAX ? 0 : lo;
    *ymax = lo == INT32_MAX ? -1 : hi;
    return PF_OK;
}

int pf_rows_add(pf_ctx* c, float* dst, const float* src, long long n)
{
    int rc;
    if ((rc = check_common(c, 1))) return rc;
    if (n < 0 || (n > 0 && (!dst || !src))) return fail(c, PF_EINVAL, "bad rows add");
    launch_rows_add(c->stream, dst, src, n);
    HIPCHK(c, hipGetLastError());
    return PF_OK;
}

int pf_rows_add_batch(pf_ctx* c, float* const* dst, const float* const* src, const long long* n,
                      int count)
{
    int rc;
    if ((rc = check_common(c, 1))) return rc;
    if (count < 0 || (count > 0 && (!dst || !src || !n))) return fail(c, PF_EINVAL, "bad rows add batch");
    for (int k = 0; k < count; k++)  // every segment checked before any is added
        if (n[k] < 0 || (n[k] > 0 && (!dst[k] || !src[k])))
            return fail(c, PF_EINVAL, "bad rows add segment %d", k);
    // launches of up to kRowsAddBatch non-empty segments; k walks the list once (empty segments
    // are skipped, so a launch may span more than kRowsAddBatch entries)
    for (int k = 0; k < count;) {
        RowsAddBatch B{};
        int m = 0;
        long long nmax = 0;
        for (; k < count && m < kRowsAddBatch; k++) {
            if (n[k] == 0) continue;
            B.dst[m] = dst[k];
            B.src[m] = src[k];
            B.n[m] = n[k];
            nmax = std::max(nmax, n[k]);
            m++;
        }
        launch_rows_add_batch(c->stream, B, m, nmax);
        HIPCHK(c, hipGetLastError());
    }
    return PF_OK;
}

int pf_fuse_seed(pf_ctx* c, const float* emap, int ew, int eh, int ec, const float* prev,
                 int out_w, int out_h, float zr0, float zr1, int level, float* buf)
{
    int rc;
    const LevelDims* L = nullptr;
    if ((rc = check_common(c, 1))) return rc;
    if (!buf) return fail(c, PF_EINVAL, "NULL buffer");
    if ((rc = level_at(c, out_w, out_h, zr0, zr1, level, &L))) return rc;
    if (level == 0) {
        if ((rc = check_emap(c, emap, ew, eh, ec))) return rc;
        launch_seed0(c->stream, emap, ew, eh, ec, 0, (const GridCol*)c->lc.cols[0].p,
                     (const GridRow*)c->lc.rows[0].p, *L, buf, 0, 1);
    } else {
        if (!prev) return fail(c, PF_EINVAL, "level %d needs the previous level's buffer", level);
        launch_upsample(c->stream, prev, 0, *L, buf, 0, 1);
    }
    HIPCHK(c, hipGetLastError());
    return PF_OK;
}

int pf_fuse_finish_level(pf_ctx* c, const float* lsum, const float* cnt, int out_w, int out_h,
                         float zr0, float zr1, int level, float* buf, uint16_t* out)
{
    int rc;
    const LevelDims* Lp = nullptr;
    if ((rc = check_common(c, 1))) return rc;
    if (!lsum || !cnt || !buf) return fail(c, PF_EINVAL, "NULL buffer");
    if ((rc = level_at(c, out_w, out_h, zr0, zr1, level, &Lp))) return rc;
    const LevelDims& L = *Lp;
    const long long st = (long long)L.w * L.h;
    if ((rc = ensure(c, c->lnorm, sizeof(float) * st))) return rc;
    if ((rc = ensure(c, c->lsum_ws, sizeof(float) * st))) return rc;
    launch_normalize(c->stream, lsum, cnt, L, (float*)c->lnorm.p);
    float* other = (float*)c->lsum_ws.p;
    // every pass stores every band row [h0, h1] of the plane it writes (pf_jacobi.hip): the second
    // plane takes the rows outside the band's interior (h0, h1), and the band comes back at the end
    const size_t rowb = sizeof(float) * (size_t)L.w;
    const int ia = std::max(L.h0 + 1, 0), ib = std::min(L.h1, L.h);  // interior rows [ia, ib)
    HIPCHK(c, hipMemcpyAsync(other, buf, rowb * ia, hipMemcpyDeviceToDevice, c->stream));
    if (ib < L.h)
        HIPCHK(c, hipMemcpyAsync(other + (size_t)ib * L.w, buf + (size_t)ib * L.w,
                                 rowb * (L.h - ib), hipMemcpyDeviceToDevice, c->stream));
    float* res = nullptr;
    if (jacobi_tcap(L) >= 1) {
        JacobiRun r{};
        r.first = 0;
        r.lnorm = (const float*)c->lnorm.p; r.a = buf; r.b = other;
        r.batch = 1;
        r.hcol = level_hcol(c, level);
        res = run_jacobi(c, L, r);
    } else {
        launch_jacobi(c->stream, buf, other, (const float*)c->lnorm.p, st, L, L.iters, 1, &res);
    }
    if ((rc = band_back(c, L, buf, res))) return rc;
    if (level == c->lc.nlevels - 1 && out) launch_quantize(c->stream, buf, st, (int)st, out, st, 1);
    HIPCHK(c, hipGetLastError());
    return PF_OK;
}

// One level's normalised targets of one panorama from every tile (the one-GPU gather,
// k_targets_patch with one-panorama blocks): the replicated levels of a one-rank row-sharded
// fusion need no partial sums.
int pf_fuse_targets(pf_ctx* c, const float* tiles, const float* coeffs, int out_w, int out_h,
                    float zr0, float zr1, int level, float* lnorm)
{
    int rc;
    const LevelDims* L = nullptr;
    if ((rc = check_common(c, 1))) return rc;
    if ((rc = check_ray_coeffs(c, "pf_fuse_targets", coeffs))) return rc;
    if (!tiles || !lnorm) return fail(c, PF_EINVAL, "NULL buffer");
    if ((rc = level_at(c, out_w, out_h, zr0, zr1, level, &L))) return rc;
    const LevelCache& lc = c->lc;
    launch_targets_patch(c->stream, (const TileGeom*)c->geom.p, (const TileBox*)lc.box[level].p,
                         (const TapBox*)lc.tapbox[level].p, c->ntiles,
                         (const int32_t*)lc.tapmap[level].p, tiles, c->tile_elems, coeffs, *L,
                         lnorm, (long long)L->w * L->h, 1, (const uint32_t*)lc.tmask[level].p,
                         (c->ntiles + 31) / 32, c->valid);
    HIPCHK(c, hipGetLastError());
    return PF_OK;
}

// One whole level of one panorama from its summed targets, seeded inside the sweeps: the
// one-call path's level (fuse_range) for a caller that gathered (lsum, cnt) itself -- the
// replicated levels of pf_dist.fuse_row_sharded.  pf_fuse_seed + pf_fuse_finish_level give the
// same planes, through a seeded full-level plane and two copies.  cnt == NULL: lsum already holds
// the normalised targets (pf_fuse_targets).
int pf_fuse_level(pf_ctx* c, const float* emap, int ew, int eh, int ec, const float* prev,
                  const float* lsum, const float* cnt, int out_w, int out_h, float zr0, float zr1,
                  int level, float* buf, uint16_t* out)
{
    int rc;
    const LevelDims* Lp = nullptr;
    if ((rc = check_common(c, 1))) return rc;
    if (!lsum || !buf) return fail(c, PF_EINVAL, "NULL buffer");
    if ((rc = level_at(c, out_w, out_h, zr0, zr1, level, &Lp))) return rc;
    const LevelDims& L = *Lp;
    const LevelCache& lc = c->lc;
    if (level == 0) {
        if ((rc = check_emap(c, emap, ew, eh, ec))) return rc;
    } else if (!prev) {
        return fail(c, PF_EINVAL, "level %d needs the previous level's buffer", level);
    }
    const long long st = (long long)L.w * L.h;
    if ((rc = ensure(c, c->lnorm, sizeof(float) * st))) return rc;
    if ((rc = ensure(c, c->lsum_ws, sizeof(float) * st))) return rc;
    const bool last = level == lc.nlevels - 1;
    uint16_t* o = last ? out : nullptr;
    if (cnt) launch_normalize(c->stream, lsum, cnt, L, (float*)c->lnorm.p);
    const float* ln = cnt ? (const float*)c->lnorm.p : lsum;
    float* other = (float*)c->lsum_ws.p;
    float* res = nullptr;
    if (jacobi_tcap(L) < 1) {  // the plain sweep form: a seeded full plane, copied, swept
        show_sweeps_plan(L, 1);
        if ((rc = pf_fuse_seed(c, emap, ew, eh, ec, prev, out_w, out_h, zr0, zr1, level, buf)))
            return rc;
        HIPCHK(c, hipMemcpyAsync(other, buf, sizeof(float) * st, hipMemcpyDeviceToDevice,
                                 c->stream));
        launch_jacobi(c->stream, buf, other, ln, st, L, L.iters, 1, &res);
        if ((rc = band_back(c, L, buf, res))) return rc;
        if (o) launch_quantize(c->stream, buf, st, (int)st, o, st, 1);
        HIPCHK(c, hipGetLastError());
        return PF_OK;
    }
    if (level == 0 && (rc = seed_tables(c, L, ew, eh, ec))) return rc;
    const JresPlan jp = jres_plan(c, L, 1, level_full(c, level));
    if (jp.on && (rc = jres_prepare(c, L, 1, jp))) return rc;
    // the rows outside the band, in both planes (the u16 rows too on the last level)
    launch_border(c->stream, level == 0 ? nullptr : prev, 0, L, buf, other, st, o, st, 1);
    JacobiRun r{};
    r.first = level == 0 ? 2 : 1;
    r.emap = emap; r.ew = ew; r.eh = eh; r.ec = ec;
    r.cols = (const GridCol*)lc.cols[level].p; r.rows = (const GridRow*)lc.rows[level].p;
    r.prev = prev;
    r.lnorm = ln; r.a = buf; r.b = other;
    r.out = o; r.ostride = st;
    r.batch = 1;
    r.hcol = level_hcol(c, level);
    r.jp = &jp;
    res = run_jacobi(c, L, r);
    if (!res) return fail(c, PF_EINVAL, "level-0 seed tables missing");
    if (!o && (rc = band_back(c, L, buf, res))) return rc;  // with o, the u16 plane is the result
    HIPCHK(c, hipGetLastError());
    return PF_OK;
}

// ---- row-band sharding of one level's sweeps (pf_dist.fuse_row_sharded) ----
int pf_fuse_normalize(pf_ctx* c, const float* lsum, const float* cnt, int out_w, int out_h,
                      float zr0, float zr1, int level, float* lnorm)
{
    int rc;
    const LevelDims* L = nullptr;
    if ((rc = check_common(c, 1))) return rc;
    if (!lsum || !cnt || !lnorm) return fail(c, PF_EINVAL, "NULL buffer");
    if ((rc = level_at(c, out_w, out_h, zr0, zr1, level, &L))) return rc;
    launch_normalize(c->stream, lsum, cnt, *L, lnorm);
    HIPCHK(c, hipGetLastError());
    return PF_OK;
}

int pf_fuse_multicover(pf_ctx* c, const float* tiles, const float* coeffs, int t0, int t1,
                       int out_w, int out_h, float zr0, float zr1, int level, float* contrib,
                       int* npairs)
{
    int rc;
    const LevelDims* L = nullptr;
    if ((rc = check_common(c, 1))) return rc;
    if ((rc = check_unmasked(c, "pf_fuse_multicover"))) return rc;
    if ((rc = check_ray_coeffs(c, "pf_fuse_multicover", coeffs))) return rc;
    if ((rc = level_at(c, out_w, out_h, zr0, zr1, level, &L))) return rc;
    const LevelCache& lc = c->lc;
    if (npairs) *npairs = lc.nmc[level];
    if (!contrib || lc.nmc[level] == 0) return PF_OK;
    if (!tiles) return fail(c, PF_EINVAL, "NULL tiles");
    if ((rc = check_tile_range(c, t0, t1))) return rc;
    launch_multicover(c->stream, (const TileGeom*)c->geom.p, (const int2*)lc.mcpairs[level].p,
                      lc.nmc[level], t0, t1, (const GridCol*)lc.cols[level].p,
                      (const GridRow*)lc.rows[level].p, tiles, coeffs, *L, contrib);
    HIPCHK(c, hipGetLastError());
    return PF_OK;
}

int pf_fuse_multicover_patch(pf_ctx* c, int out_w, int out_h, float zr0, float zr1, int level,
                             const float* contrib, float* lsum)
{
    int rc;
    const LevelDims* L = nullptr;
    if ((rc = check_common(c, 1))) return rc;
    if ((rc = check_unmasked(c, "pf_fuse_multicover_patch"))) return rc;
    if ((rc = level_at(c, out_w, out_h, zr0, zr1, level, &L))) return rc;
    const LevelCache& lc = c->lc;
    if (lc.nmc[level] == 0) return PF_OK;
    if (!contrib || !lsum) return fail(c, PF_EINVAL, "NULL buffer");
    launch_multicover_patch(c->stream, (const int2*)lc.mcpairs[level].p, lc.nmc[level], contrib,
                            lsum);
    HIPCHK(c, hipGetLastError());
    return PF_OK;
}

int pf_fuse_border(pf_ctx* c, const float* prev, int out_w, int out_h, float zr0, float zr1,
                   int level, float* a, float* b, uint16_t* out)
{
    int rc;
    const LevelDims* L = nullptr;
    if ((rc = check_common(c, 1))) return rc;
    if ((rc = level_at(c, out_w, out_h, zr0, zr1, level, &L))) return rc;
    const LevelCache& lc = c->lc;
    if (level > 0 && !prev) return fail(c, PF_EINVAL, "level %d needs the previous level", level);
    const bool last = level == lc.nlevels - 1;
    if (last ? !out : (!a || !b)) return fail(c, PF_EINVAL, "NULL buffer");
    const long long st = (long long)L->w * L->h;
    const long long pst = level > 0 ? (long long)lc.dims[level - 1].w * lc.dims[level - 1].h : 0;
    launch_border(c->stream, level == 0 ? nullptr : prev, pst, *L, a, b, st, last ? out : nullptr,
                  st, 1);  // last level: a / b (if given) get the rows h0-1 and h1+1
    HIPCHK(c, hipGetLastError());
    return PF_OK;
}

int pf_fuse_band_plan(pf_ctx* c, int out_w, int out_h, float zr0, float zr1, int level,
                      int nbands, int* T, int cap)
{
    int rc;
    const LevelDims* L = nullptr;
    if ((rc = check_common(c, 1))) return rc;
    const bool count_only = !T && cap == 0;  // the number of passes; 0, not an error, where none
    if ((!count_only && (!T || cap < 1)) || nbands < 1)
        return fail(c, PF_EINVAL, "pf_fuse_band_plan: bad arguments");
    if ((rc = level_at(c, out_w, out_h, zr0, zr1, level, &L))) return rc;
    if (jacobi_tcap(*L) < 1) {
        if (count_only) return 0;
        // jacobi_tcap: the halo rows of a pass must stay inside [1, h-2], and a strip inside a row
        if (std::min(L->h0 - 1, L->h - 2 - L->h1) < 1)
            return fail(c, PF_EINVAL, "level %d: the zenith band leaves no room for band passes",
                        level);
        return fail(c, PF_EINVAL,
                    "level %d: no band passes at width %d (odd, or too narrow for a strip): the "
                    "level runs on the per-sweep engine (pf_fuse_level, pf_fuse_finish_level)",
                    level, L->w);
    }
    const int band = L->h1 - L->h0 + 1;
    // the sweep depths depend only on (level, nbands): every rank derives the same plan
    std::vector<PassPlan> plan = plan_level(c, *L, jacobi_tcap(*L), 1, level_full(c, level),
                                            (band + nbands - 1) / nbands);
    if (count_only) return (int)plan.size();
    if ((int)plan.size() > cap) return fail(c, PF_EINVAL, "plan of %zu passes > cap %d", plan.size(), cap);
    for (size_t i = 0; i < plan.size(); i++) T[i] = plan[i].T;
    return (int)plan.size();
}

int pf_fuse_band_pass(pf_ctx* c, const float* emap, int ew, int eh, int ec, const float* prev,
                      const float* lnorm, int src_mode, const float* src, float* dst,
                      uint16_t* out, int out_w, int out_h, float zr0, float zr1, int level, int T,
                      int row0, int row1)
{
    int rc;
    const LevelDims* Lp = nullptr;
    if ((rc = check_common(c, 1))) return rc;
    if ((rc = level_at(c, out_w, out_h, zr0, zr1, level, &Lp))) return rc;
    const LevelDims& L = *Lp;
    const LevelCache& lc = c->lc;
    if (!lnorm || (!dst && !out)) return fail(c, PF_EINVAL, "NULL buffer");
    if (src_mode < 0 || src_mode > 2) return fail(c, PF_EINVAL, "src_mode %d", src_mode);
    if (src_mode == 0 && !src) return fail(c, PF_EINVAL, "src_mode 0 needs src");
    if (src_mode == 1 && (level == 0 || !prev)) return fail(c, PF_EINVAL, "src_mode 1 needs prev");
    if (src_mode == 2 && (level != 0 || (rc = check_emap(c, emap, ew, eh, ec))))
        return rc ? rc : fail(c, PF_EINVAL, "src_mode 2 (seed) is level 0 only");
    if (T < 1 || T > jacobi_tcap(L) || !jstream_supported_T(T))
        return fail(c, PF_EINVAL, "pass depth %d not available at level %d", T, level);
    if (row0 < L.h0 || row1 > L.h1 + 1 || row0 >= row1)
        return fail(c, PF_EINVAL, "rows [%d,%d) outside the band [%d,%d]", row0, row1, L.h0, L.h1);
    const bool fast = level_full(c, level);
    if (src_mode == 2 && (rc = seed_tables(c, L, ew, eh, ec))) return rc;
    JacobiRun r{};
    r.first = src_mode;
    r.emap = emap; r.ew = ew; r.eh = eh; r.ec = ec;
    r.cols = (const GridCol*)lc.cols[level].p; r.rows = (const GridRow*)lc.rows[level].p;
    r.prev = prev;
    r.lnorm = lnorm;
    r.out = out; r.ostride = (long long)L.w * L.h;
    r.hcol = level_hcol(c, level);
    JacobiPass P = jacobi_pass(c, L, r);
    P.row_lo = row0;
    P.row_hi = row1;
    set_pass_shape(P, T, row1 - row0, plan_band_pass(c, L, T, row1 - row0, fast).nchunks);
    P.src_mode = src_mode;
    P.src = src;
    P.dst = dst;
    P.out_mode = out ? 1 : 0;
    launch_jstream(c->stream, P, T, 1, fast);
    HIPCHK(c, hipGetLastError());
    return PF_OK;
}

int pf_probe_taps(pf_ctx* c, int out_w, int out_h, float zr0, float zr1, int level,
                  int32_t* tap_index)
{
    int rc;
    const LevelDims* L = nullptr;
    if ((rc = check_common(c, 1))) return rc;
    if (!tap_index) return fail(c, PF_EINVAL, "NULL buffer");
    if ((rc = level_at(c, out_w, out_h, zr0, zr1, level, &L))) return rc;
    const LevelCache& lc = c->lc;
    launch_probe_taps(c->stream, (const TileGeom*)c->geom.p, (const TileBox*)lc.box[level].p,
                      c->ntiles, (const GridCol*)lc.cols[level].p, (const GridRow*)lc.rows[level].p,
                      *L, tap_index);
    HIPCHK(c, hipGetLastError());
    return PF_OK;
}

}  // extern "C"
