// pf_disp_api.hip -- the entry points of the disparity-tile path (MiDaS / DPT tiles: relative
// inverse depth in 0-1): pf_register_disparity, pf_disparity_transform, pf_merge_disparity.
#include "pf_ctx.hpp"

using namespace pf;

extern "C" {

int pf_register_disparity(pf_ctx* c, const float* emap, int ew, int eh, int ec, float* tiles,
                          int batch, float zr0, float zr1, int apply, float* coeffs,
                          double* coeffs64, double* summary)
{
    int rc;
    if ((rc = check_common(c, batch))) return rc;
    if ((rc = check_unmasked(c, "pf_register_disparity"))) return rc;
    if ((rc = check_emap(c, emap, ew, eh, ec))) return rc;
    if (!tiles) return fail(c, PF_EINVAL, "tiles is NULL");
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
    if (!sidx) return fail(c, PF_EHIP, "pf_register_disparity: no sample-index table");
    if (c->tile_depth == PF_TILE_DEPTH_PLANAR) {  // the fit and D2DTransform with the ray factor
        const float* kfs = reg_sample_kf(c, ew, eh, ec);
        if (!kfs) return fail(c, PF_EHIP, "pf_register_disparity: no sample ray-factor table");
        StageTimer t(c, PF_STAGE_REGISTER,
                     batch * (12.0 * nsamp + (apply ? 8.0 * (double)c->tile_elems / c->tile_c : 0.0)),
                     apply ? 2 : 1);
        launch_register_disp_planar(c->stream, (const TileGeom*)c->geom.p,
                                    (const RegGrid*)c->reg.p, c->ntiles, emap,
                                    (long long)ew * eh * ec, tiles, c->tile_elems, sidx, kfs, cf,
                                    coeffs64, summary, batch, c->loss_kind, c->loss_a);
        if (apply)
            launch_apply_disp_planar(c->stream, (const TileGeom*)c->geom.p,
                                     (const RayTile*)c->ray.p, (const double*)c->ray_tab.p,
                                     c->ntiles, c->tile_elems / c->tile_c, tiles, tiles,
                                     c->tile_elems, cf, batch);
    } else {
        StageTimer t(c, PF_STAGE_REGISTER,
                     batch * (8.0 * nsamp + (apply ? 8.0 * (double)c->tile_elems / c->tile_c : 0.0)),
                     apply ? 2 : 1);
        launch_register_disp(c->stream, (const TileGeom*)c->geom.p, (const RegGrid*)c->reg.p,
                             c->ntiles, emap, (long long)ew * eh * ec, tiles, c->tile_elems, sidx,
                             cf, coeffs64, summary, batch, c->loss_kind, c->loss_a);
        if (apply)
            launch_apply_disp(c->stream, (const TileGeom*)c->geom.p, c->ntiles,
                              c->tile_elems / c->tile_c, tiles, c->tile_elems, cf, batch);
    }
    HIPCHK(c, hipGetLastError());
    return PF_OK;
}

int pf_disparity_transform(pf_ctx* c, float* data, long long npix, int channels, const float* abcd)
{
    int rc;
    if ((rc = check_device(c))) return rc;
    if (!data || !abcd || npix < 0 || channels < 1)
        return fail(c, PF_EINVAL, "pf_disparity_transform: bad arguments");
    if (npix == 0) return PF_OK;
    launch_disp_map(c->stream, data, npix, channels, abcd);
    HIPCHK(c, hipGetLastError());
    return PF_OK;
}

int pf_merge_disparity(pf_ctx* c, const float* emap, int ew, int eh, int ec, const float* tiles,
                       int batch, int out_w, float zr0, float zr1, float* coeffs, uint16_t* out)
{
    int rc;
    if ((rc = check_common(c, batch))) return rc;
    if ((rc = check_unmasked(c, "pf_merge_disparity"))) return rc;
    if ((rc = check_emap(c, emap, ew, eh, ec))) return rc;
    if (!tiles || !out) return fail(c, PF_EINVAL, "tiles/out is NULL");
    const size_t bytes = sizeof(float) * (size_t)c->tile_elems * batch;
    if ((rc = ensure(c, c->disp_tiles, bytes))) return rc;
    float* copy = (float*)c->disp_tiles.p;
    HIPCHK(c, hipMemcpyAsync(copy, tiles, bytes, hipMemcpyDeviceToDevice, c->stream));
    if ((rc = pf_register_disparity(c, emap, ew, eh, ec, copy, batch, zr0, zr1, 1, coeffs, nullptr,
                                    nullptr)))
        return rc;
    return pf_fuse(c, emap, ew, eh, ec, copy, nullptr, batch, out_w, out_w / 2, zr0, zr1, out);
}

}  // extern "C"
