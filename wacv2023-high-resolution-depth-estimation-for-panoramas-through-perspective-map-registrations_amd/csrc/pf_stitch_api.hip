// pf_stitch_api.hip -- pf_stitch (the direct tile stitch, Depth.cpp:817-865), and the Laplacian
// self-check of SolveDepthAll (Depth.cpp:1738-1758): pf_laplacian_residual on given planes and
// pf_fuse_check, the fusion of one panorama with the check after every level.
#include "pf_ctx.hpp"

#include <cmath>

using namespace pf;

extern "C" {

int pf_stitch(pf_ctx* c, const float* tiles, const float* coeffs, int batch, int out_w, int out_h,
              uint16_t* out)
{
    int rc;
    if ((rc = check_common(c, batch))) return rc;
    if ((rc = check_ray_coeffs(c, "pf_stitch", coeffs))) return rc;
    if (!tiles || !out) return fail(c, PF_EINVAL, "tiles/out is NULL");
    if (out_w < 2 || out_h < 2 || (long long)out_w * out_h >= (1LL << 31) - 512)
        return fail(c, PF_EINVAL, "output %dx%d out of range", out_w, out_h);
    if (c->st_key[0] != out_w || c->st_key[1] != out_h) {  // the map of this layout and size
        c->st_key[0] = c->st_key[1] = 0;
        std::vector<SmoothBox> boxes(c->ntiles);
        for (int p = 0; p < c->ntiles; p++) {  // :834-837, per tile instead of per pixel
            const pf_window& r = c->rng[p];
            SmoothBox b{};
            b.x0 = (int)round((double)r.az_left / (2 * PF_MYPI) * (double)(out_w - 1));
            b.x1 = (int)round((double)r.az_right / (2 * PF_MYPI) * (double)(out_w - 1));
            b.y0 = (int)round((double)r.zen_top / PF_MYPI * (double)(out_h - 1));
            b.y1 = (int)round((double)r.zen_down / PF_MYPI * (double)(out_h - 1));
            boxes[p] = b;  // a box that leaves the grid only covers the part inside it
        }
        LevelDims L{};
        L.w = out_w;
        L.h = out_h;
        std::vector<GridCol> cols;
        std::vector<GridRow> rows;
        grid_tables(L, cols, rows);
        const long long n = (long long)out_w * out_h;
        if ((rc = upload(c, c->st_box, boxes))) return rc;
        if ((rc = upload(c, c->st_cols, cols))) return rc;
        if ((rc = upload(c, c->st_rows, rows))) return rc;
        if ((rc = ensure(c, c->st_src, sizeof(int2) * n))) return rc;
        launch_stitch_map(c->stream, (const TileGeom*)c->geom.p, (const SmoothBox*)c->st_box.p,
                          c->ntiles, (const GridCol*)c->st_cols.p, (const GridRow*)c->st_rows.p,
                          out_w, out_h, (int2*)c->st_src.p);
        HIPCHK(c, hipGetLastError());
        c->st_key[0] = out_w;
        c->st_key[1] = out_h;
    }
    if (c->valid.on)  // the first VALID tile depends on the data: the tables, not the cached map
        launch_stitch_valid(c->stream, (const TileGeom*)c->geom.p, (const SmoothBox*)c->st_box.p,
                            c->ntiles, (const GridCol*)c->st_cols.p, (const GridRow*)c->st_rows.p,
                            tiles, c->tile_elems, coeffs, out_w, out_h, c->valid, out, batch);
    else
        launch_stitch(c->stream, (const TileGeom*)c->geom.p, c->ntiles, (const int2*)c->st_src.p,
                      tiles, c->tile_elems, coeffs, out_w, out_h, out, batch);
    HIPCHK(c, hipGetLastError());
    return PF_OK;
}

int pf_laplacian_residual(pf_ctx* c, const float* buf, const float* lnorm, int w, int h, int h0,
                          int h1, int batch, float* err)
{
    int rc;
    if ((rc = check_device(c))) return rc;
    if (batch <= 0 || batch > 65535) return fail(c, PF_EINVAL, "batch %d out of range", batch);
    if (!buf || !lnorm || !err) return fail(c, PF_EINVAL, "NULL buffer");
    if (w < 3 || h < 3 || (long long)w * h >= (1LL << 31) - 512)
        return fail(c, PF_EINVAL, "plane %dx%d out of range", w, h);
    if (h0 < 0 || h1 > h - 1 || h0 + 2 > h1)
        return fail(c, PF_EINVAL, "rows (%d, %d) of %d: the check needs 0 <= h0, h0 + 2 <= h1 "
                    "<= h - 1", h0, h1, h);
    launch_lap_residual(c->stream, buf, lnorm, w, h, h0, h1, batch, err);
    HIPCHK(c, hipGetLastError());
    return PF_OK;
}

int pf_fuse_check(pf_ctx* c, const float* emap, int ew, int eh, int ec, const float* tiles,
                  const float* coeffs, int out_w, int out_h, float zr0, float zr1, float* err,
                  uint16_t* out)
{
    int rc;
    if ((rc = check_common(c, 1))) return rc;
    if ((rc = check_ray_coeffs(c, "pf_fuse_check", coeffs))) return rc;
    if ((rc = check_emap(c, emap, ew, eh, ec))) return rc;
    if (!tiles || !err) return fail(c, PF_EINVAL, "tiles/err is NULL");
    if ((rc = jres_check(c))) return rc;  // an earlier fusion's timeout, once it has landed
    if ((rc = prepare_levels(c, out_w, out_h, zr0, zr1))) return rc;
    const int nlevels = c->lc.nlevels;
    const long long plane = (long long)out_w * out_h;
    // two level planes (the previous level's and this one's) and the level's targets; sized
    // before any is used (a growing buffer is freed first)
    for (int k = 0; k < 3; k++)
        if ((rc = ensure(c, c->buf[k], sizeof(float) * plane))) return rc;
    float* prev = nullptr;
    float* cur = (float*)c->buf[0].p;
    float* const ln = (float*)c->buf[2].p;
    for (int l = 0; l < nlevels; l++) {
        const LevelDims L = c->lc.dims[l];
        if ((rc = pf_fuse_targets(c, tiles, coeffs, out_w, out_h, zr0, zr1, l, ln))) return rc;
        if ((rc = pf_fuse_level(c, emap, ew, eh, ec, prev, ln, nullptr, out_w, out_h, zr0, zr1,
                                l, cur, nullptr)))
            return rc;
        if ((rc = pf_laplacian_residual(c, cur, ln, L.w, L.h, L.h0, L.h1, 1, err + l))) return rc;
        prev = cur;
        cur = cur == (float*)c->buf[0].p ? (float*)c->buf[1].p : (float*)c->buf[0].p;
    }
    if (out) launch_quantize(c->stream, prev, plane, (int)plane, out, plane, 1);
    HIPCHK(c, hipGetLastError());
    return PF_OK;
}

}  // extern "C"
