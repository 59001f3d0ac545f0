// pf_weight_api.hip -- the entry points of the per-pixel tile weights: pf_tile_tent_weights,
// pf_register_weighted, pf_fuse_weighted, pf_merge_weighted, and the disparity path's weighted
// forms pf_tile_range_weights, pf_register_disparity_weighted, pf_merge_disparity_weighted
// (include/panofuse.h has the contract).  New entry points only: pf_register / pf_fuse / pf_merge /
// pf_register_disparity / pf_merge_disparity launch what they always did.
#include "pf_ctx.hpp"

using namespace pf;

namespace {

// The weighted forms exist for ray-distance tiles under plain least squares only: the validity
// rule (which weights in {0, 1} restate), a loss and planar-depth tiles are refused, never
// silently ignored.
int check_weight_modes(pf_ctx* c, const char* entry)
{
    int rc;
    if (!c) return PF_EINVAL;
    if ((rc = check_unmasked(c, entry))) return rc;
    if ((rc = check_no_loss(c, entry))) return rc;
    if (c->tile_depth != PF_TILE_DEPTH_RAY)
        return fail(c, PF_ESTATE,
                    "%s has no planar-depth form: call pf_set_tile_depth(ctx, PF_TILE_DEPTH_RAY) "
                    "first",
                    entry);
    return PF_OK;
}

// weights / wbatch of a weighted call; *wstride = the panorama stride of the weight plane.
int check_weights(pf_ctx* c, const char* entry, const float* weights, int wbatch, int batch,
                  long long* wstride)
{
    if (!weights) return fail(c, PF_EINVAL, "%s: weights is NULL", entry);
    if (wbatch != 1 && wbatch != batch)
        return fail(c, PF_EINVAL, "%s: wbatch %d is neither 1 nor the batch %d", entry, wbatch,
                    batch);
    *wstride = wbatch == 1 ? 0 : c->tile_elems;
    return PF_OK;
}

int check_lm(pf_ctx* c, const char* entry)
{
    if (c->solver != PF_SOLVER_LM)
        return fail(c, PF_EINVAL, "%s needs PF_SOLVER_LM (pf_set_solver): the weighted fit is "
                    "degree 3 by the LM only", entry);
    return PF_OK;
}

int check_fusable(pf_ctx* c, const char* entry)
{
    if (c->tile_elems > targets_weighted_max_elems())
        return fail(c, PF_EINVAL, "%s: the weighted gather takes layouts of at most 2^30 tile "
                    "elements per panorama (got %lld)", entry, c->tile_elems);
    return PF_OK;
}

int register_weighted(pf_ctx* c, const float* emap, int ew, int eh, int ec, float* tiles,
                      const float* weights, long long wstride, int batch, float zr0, float zr1,
                      int apply, float* coeffs, double* coeffs64, double* summary)
{
    int rc;
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
    if (!sidx) return fail(c, PF_EHIP, "weighted registration: no sample-index table");
    const TileGeom* geom = (const TileGeom*)c->geom.p;
    StageTimer t(c, PF_STAGE_REGISTER,
                 batch * (12.0 * nsamp + (apply ? 8.0 * (double)c->tile_elems / c->tile_c : 0.0)),
                 apply ? 2 : 1);
    launch_register_weighted(c->stream, geom, (const RegGrid*)c->reg.p, c->ntiles, emap,
                             (long long)ew * eh * ec, tiles, c->tile_elems, weights, wstride, cf,
                             coeffs64, summary, batch, sidx);
    if (apply)
        launch_apply_cubic(c->stream, geom, c->ntiles, c->tile_elems / c->tile_c, tiles,
                           c->tile_elems, cf, batch);
    HIPCHK(c, hipGetLastError());
    return PF_OK;
}

// fuse_impl with the weight plane on the context for the duration of the call.
int fuse_weighted(pf_ctx* c, const float* emap, int ew, int eh, int ec, const float* tiles,
                  const float* weights, long long wstride, const float* coeffs, int batch,
                  int out_w, int out_h, float zr0, float zr1, uint16_t* out)
{
    c->wts = weights;
    c->wts_stride = wstride;
    const int rc = fuse_impl(c, emap, ew, eh, ec, tiles, coeffs, batch, out_w, out_h, zr0, zr1, out);
    c->wts = nullptr;
    c->wts_stride = 0;
    return rc;
}

// The disparity path's weighted forms run under plain least squares without the validity rule
// (which weights in {0, 1} restate); planar-depth tiles are honoured.  Checked before anything else.
int check_disp_weight_modes(pf_ctx* c, const char* entry)
{
    if (!c) return PF_EINVAL;
    if (c->valid.on)
        return fail(c, PF_ESTATE,
                    "%s does not run under the tile validity rule: call pf_set_tile_validity(ctx, "
                    "PF_VALID_ALL, 0, 0) first and pass the rule as weights (pf_tile_range_weights)",
                    entry);
    if (c->loss_kind != PF_LOSS_NONE)
        return fail(c, PF_ESTATE,
                    "%s has no robust form: call pf_set_register_loss(ctx, PF_LOSS_NONE, 0) first",
                    entry);
    return PF_OK;
}

// pf_register_disparity's fit with a weight per sample (k_register_disp_weighted): the samples'
// usable weights go to the context's table first (k_disp_sample_weights), one row per panorama.
int register_disparity_weighted(pf_ctx* c, const float* emap, int ew, int eh, int ec, float* tiles,
                                const float* weights, long long wstride, int batch, float zr0,
                                float zr1, int apply, float* coeffs, double* coeffs64,
                                double* summary)
{
    int rc;
    if ((rc = prepare_registration(c, zr0, zr1))) return rc;
    if ((rc = check_reg_grids(c, nullptr))) return rc;
    float* cf = coeffs;
    if (!cf) {
        if ((rc = ensure(c, c->coeffs, sizeof(float) * 4 * c->ntiles * batch))) return rc;
        cf = (float*)c->coeffs.p;
    }
    long long nsamp = 0;
    int maxn = 0;
    for (const RegGrid& g : c->reg_h) {
        const int k = (g.cols + 1) * (g.rows + 1);
        nsamp += k;
        maxn = k > maxn ? k : maxn;
    }
    const int2* sidx = reg_sample_index(c, ew, eh, ec);  // before the stage timer: built once
    if (!sidx) return fail(c, PF_EHIP, "pf_register_disparity_weighted: no sample-index table");
    const bool planar = c->tile_depth == PF_TILE_DEPTH_PLANAR;
    const float* kfs = nullptr;
    if (planar && !(kfs = reg_sample_kf(c, ew, eh, ec)))
        return fail(c, PF_EHIP, "pf_register_disparity_weighted: no sample ray-factor table");
    if ((rc = ensure(c, c->disp_ws, sizeof(float) * (size_t)nsamp * batch))) return rc;
    float* ws = (float*)c->disp_ws.p;
    const TileGeom* geom = (const TileGeom*)c->geom.p;
    const RegGrid* grids = (const RegGrid*)c->reg.p;
    const long long estride = (long long)ew * eh * ec;
    StageTimer t(c, PF_STAGE_REGISTER,
                 batch * ((planar ? 24.0 : 20.0) * (double)nsamp +
                          (apply ? 8.0 * (double)c->tile_elems / c->tile_c : 0.0)),
                 apply ? 3 : 2);
    launch_disp_sample_weights(c->stream, geom, grids, c->ntiles, maxn, emap, estride, tiles,
                               c->tile_elems, weights, wstride, sidx, ws, nsamp, batch);
    launch_register_disp_weighted(c->stream, geom, grids, c->ntiles, emap, estride, tiles,
                                  c->tile_elems, sidx, kfs, ws, nsamp, cf, coeffs64, summary,
                                  batch);
    if (apply) {
        if (planar)
            launch_apply_disp_planar(c->stream, geom, (const RayTile*)c->ray.p,
                                     (const double*)c->ray_tab.p, c->ntiles,
                                     c->tile_elems / c->tile_c, tiles, tiles, c->tile_elems, cf,
                                     batch);
        else
            launch_apply_disp(c->stream, geom, c->ntiles, c->tile_elems / c->tile_c, tiles,
                              c->tile_elems, cf, batch);
    }
    HIPCHK(c, hipGetLastError());
    return PF_OK;
}

}  // namespace

extern "C" {

int pf_tile_range_weights(pf_ctx* c, const float* tiles, int batch, float lo, float hi,
                          float* weights)
{
    int rc;
    if ((rc = check_common(c, batch))) return rc;
    if (!tiles || !weights)
        return fail(c, PF_EINVAL, "pf_tile_range_weights: tiles/weights is NULL");
    launch_range_weights(c->stream, tiles, c->tile_elems / c->tile_c * batch, c->tile_c, lo, hi,
                         weights);
    HIPCHK(c, hipGetLastError());
    return PF_OK;
}

int pf_register_disparity_weighted(pf_ctx* c, const float* emap, int ew, int eh, int ec,
                                   float* tiles, const float* weights, int wbatch, int batch,
                                   float zr0, float zr1, int apply, float* coeffs,
                                   double* coeffs64, double* summary)
{
    int rc;
    long long wstride = 0;
    if ((rc = check_disp_weight_modes(c, "pf_register_disparity_weighted"))) return rc;
    if ((rc = check_common(c, batch))) return rc;
    if ((rc = check_emap(c, emap, ew, eh, ec))) return rc;
    if (!tiles) return fail(c, PF_EINVAL, "tiles is NULL");
    if ((rc = check_weights(c, "pf_register_disparity_weighted", weights, wbatch, batch, &wstride)))
        return rc;
    return register_disparity_weighted(c, emap, ew, eh, ec, tiles, weights, wstride, batch, zr0,
                                       zr1, apply, coeffs, coeffs64, summary);
}

int pf_merge_disparity_weighted(pf_ctx* c, const float* emap, int ew, int eh, int ec,
                                const float* tiles, const float* weights, int wbatch, int batch,
                                int out_w, float zr0, float zr1, float* coeffs, uint16_t* out)
{
    int rc;
    long long wstride = 0;
    if ((rc = check_disp_weight_modes(c, "pf_merge_disparity_weighted"))) return rc;
    if ((rc = check_common(c, batch))) return rc;
    if ((rc = check_emap(c, emap, ew, eh, ec))) return rc;
    if (!tiles || !out) return fail(c, PF_EINVAL, "tiles/out is NULL");
    if ((rc = check_weights(c, "pf_merge_disparity_weighted", weights, wbatch, batch, &wstride)))
        return rc;
    if ((rc = check_fusable(c, "pf_merge_disparity_weighted"))) return rc;
    if ((rc = jres_check(c))) return rc;
    const size_t bytes = sizeof(float) * (size_t)c->tile_elems * batch;
    if ((rc = ensure(c, c->disp_tiles, bytes))) return rc;
    float* copy = (float*)c->disp_tiles.p;
    HIPCHK(c, hipMemcpyAsync(copy, tiles, bytes, hipMemcpyDeviceToDevice, c->stream));
    if ((rc = register_disparity_weighted(c, emap, ew, eh, ec, copy, weights, wstride, batch, zr0,
                                          zr1, 1, coeffs, nullptr, nullptr)))
        return rc;
    // the transformed copy is ray distance: fused without coefficients, a tile left with NaN
    // coefficients is all NaN and drops out of every pixel (the staged-NaN rule of the gather)
    return fuse_weighted(c, emap, ew, eh, ec, copy, weights, wstride, nullptr, batch, out_w,
                         out_w / 2, zr0, zr1, out);
}

int pf_tile_tent_weights(pf_ctx* c, float* weights)
{
    int rc;
    if ((rc = check_weight_modes(c, "pf_tile_tent_weights"))) return rc;
    if ((rc = check_common(c, 1))) return rc;
    if (!weights) return fail(c, PF_EINVAL, "pf_tile_tent_weights: weights is NULL");
    launch_tent_weights(c->stream, (const TileGeom*)c->geom.p, c->ntiles,
                        c->tile_elems / c->tile_c, weights);
    HIPCHK(c, hipGetLastError());
    return PF_OK;
}

int pf_register_weighted(pf_ctx* c, const float* emap, int ew, int eh, int ec, float* tiles,
                         const float* weights, int wbatch, int batch, float zr0, float zr1,
                         int apply, float* coeffs, double* coeffs64, double* summary)
{
    int rc;
    long long wstride = 0;
    if ((rc = check_weight_modes(c, "pf_register_weighted"))) return rc;
    if ((rc = check_common(c, batch))) return rc;
    if ((rc = check_emap(c, emap, ew, eh, ec))) return rc;
    if (!tiles) return fail(c, PF_EINVAL, "tiles is NULL");
    if ((rc = check_weights(c, "pf_register_weighted", weights, wbatch, batch, &wstride))) return rc;
    if ((rc = check_lm(c, "pf_register_weighted"))) return rc;
    return register_weighted(c, emap, ew, eh, ec, tiles, weights, wstride, batch, zr0, zr1, apply,
                             coeffs, coeffs64, summary);
}

int pf_fuse_weighted(pf_ctx* c, const float* emap, int ew, int eh, int ec, const float* tiles,
                     const float* weights, int wbatch, const float* coeffs, int batch, int out_w,
                     int out_h, float zr0, float zr1, uint16_t* out)
{
    int rc;
    long long wstride = 0;
    if ((rc = check_weight_modes(c, "pf_fuse_weighted"))) return rc;
    if ((rc = check_common(c, batch))) return rc;
    if ((rc = check_emap(c, emap, ew, eh, ec))) return rc;
    if (!tiles || !out) return fail(c, PF_EINVAL, "tiles/out is NULL");
    if ((rc = check_weights(c, "pf_fuse_weighted", weights, wbatch, batch, &wstride))) return rc;
    if ((rc = check_fusable(c, "pf_fuse_weighted"))) return rc;
    if ((rc = jres_check(c))) return rc;  // an earlier fusion's timeout, once it has landed
    return fuse_weighted(c, emap, ew, eh, ec, tiles, weights, wstride, coeffs, batch, out_w, out_h,
                         zr0, zr1, out);
}

int pf_merge_weighted(pf_ctx* c, const float* emap, int ew, int eh, int ec, const float* tiles,
                      const float* weights, int wbatch, int batch, int out_w, float zr0,
                      float zr1, float* coeffs, uint16_t* out)
{
    int rc;
    long long wstride = 0;
    if ((rc = check_weight_modes(c, "pf_merge_weighted"))) return rc;
    if ((rc = check_common(c, batch))) return rc;
    if ((rc = check_emap(c, emap, ew, eh, ec))) return rc;
    if (!tiles || !out) return fail(c, PF_EINVAL, "tiles/out is NULL");
    if ((rc = check_weights(c, "pf_merge_weighted", weights, wbatch, batch, &wstride))) return rc;
    if ((rc = check_lm(c, "pf_merge_weighted"))) return rc;
    if ((rc = check_fusable(c, "pf_merge_weighted"))) return rc;
    if ((rc = jres_check(c))) return rc;
    float* cf = coeffs;
    if (!cf) {
        if ((rc = ensure(c, c->coeffs, sizeof(float) * 4 * c->ntiles * batch))) return rc;
        cf = (float*)c->coeffs.p;
    }
    if ((rc = register_weighted(c, emap, ew, eh, ec, const_cast<float*>(tiles), weights, wstride,
                                batch, zr0, zr1, 0, cf, nullptr, nullptr)))
        return rc;
    return fuse_weighted(c, emap, ew, eh, ec, tiles, weights, wstride, cf, batch, out_w, out_w / 2,
                         zr0, zr1, out);
}

}  // extern "C"
