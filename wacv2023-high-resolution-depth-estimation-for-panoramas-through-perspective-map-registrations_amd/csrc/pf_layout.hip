// pf_layout.hip -- host-side preparation done once per layout / fusion level (all tiny): the tile
// windows (PerspectiveMap::SetWindow, Depth.cpp:120-155), the per-level tile boxes
// (Depth.cpp:1497-1562) and the separable trig tables of the fusion and registration grids,
// computed with glibc's sincosf/tanf exactly as the reference calls them.  Everything per
// panorama runs on the GPU.
#include "pf_ctx.hpp"
#include "pf_geom.hpp"
#include "pf_ray.hpp"

#include <algorithm>
#include <cmath>

using namespace pf;

// ---------------------------------------------------------------------------------------------
// Host geometry: PerspectiveMap::SetWindow in Imath Vec3<float> semantics (pf_geom.hpp).
namespace {
TileGeom set_window(const pf_window& f, int w, int h, int ch)
{  // PerspectiveMap::SetWindow, Depth.cpp:120-155
    using namespace pfgeom;
    const Window win = pfgeom::set_window(f.az_left, f.az_right, f.zen_top, f.zen_down);
    TileGeom g{};
    g.middle[0] = win.middle.x; g.middle[1] = win.middle.y; g.middle[2] = win.middle.z;
    g.hedge[0] = win.hedge.x; g.hedge[1] = win.hedge.y; g.hedge[2] = win.hedge.z;
    g.vedge[0] = win.vedge.x; g.vedge[1] = win.vedge.y; g.vedge[2] = win.vedge.z;
    g.corner0[0] = win.corner0.x; g.corner0[1] = win.corner0.y; g.corner0[2] = win.corner0.z;
    const V3 p0mp = {win.middle.x - 0.0f, win.middle.y - 0.0f, win.middle.z - 0.0f};  // p0 - p
    g.mm = dot(p0mp, win.middle);
    g.hl = length(win.hedge);
    g.vl = length(win.vedge);
    g.w = w;
    g.h = h;
    g.c = ch;
    return g;
}

// RGB camera of SaveCubeMap (Main.cpp:246-269: gluLookAt toward the window centre, up = z;
// gluPerspective fovy / aspect), in double.
RgbCam rgb_cam(const pf_window& f)
{
    float azc = (f.az_right + f.az_left) / 2, zenc = (f.zen_down + f.zen_top) / 2;
    float fovx = (float)((f.az_right - f.az_left) / PF_MYPI * 180.0);
    float fovy = (float)((f.zen_down - f.zen_top) / PF_MYPI * 180.0);
    float aspect = (float)(tan(fovx / 180.0 * PF_MYPI / 2) / tan(fovy / 180.0 * PF_MYPI / 2));
    RgbCam cam{};
    double fv[3] = {cos((double)azc) * sin((double)zenc), sin((double)azc) * sin((double)zenc),
                    cos((double)zenc)};
    double fl = sqrt(fv[0] * fv[0] + fv[1] * fv[1] + fv[2] * fv[2]);
    for (int k = 0; k < 3; k++) cam.f[k] = fv[k] / fl;
    double sv[3] = {cam.f[1], -cam.f[0], 0.0};
    double sl = sqrt(sv[0] * sv[0] + sv[1] * sv[1]);
    cam.s[0] = sv[0] / sl; cam.s[1] = sv[1] / sl; cam.s[2] = 0.0;
    cam.u[0] = cam.s[1] * cam.f[2] - cam.s[2] * cam.f[1];
    cam.u[1] = cam.s[2] * cam.f[0] - cam.s[0] * cam.f[2];
    cam.u[2] = cam.s[0] * cam.f[1] - cam.s[1] * cam.f[0];
    cam.ty = tan((double)fovy / 180.0 * PF_MYPI / 2);
    cam.tx = cam.ty * (double)aspect;
    return cam;
}

LevelDims level_dims(int out_w, int out_h, float zr0, float zr1, int level)
{  // Depth.cpp:1420-1437, 1650-1675
    LevelDims L{};
    int max_level = out_w >= 4096 ? 4 : 3;
    L.nlevels = max_level;
    L.w = (int)(out_w / pow(2, max_level - 1 - level));
    L.h = (int)(out_h / pow(2, max_level - 1 - level));
    L.h0 = (int)floor((double)((float)L.h * zr0) / PF_MYPI);
    L.h1 = (int)ceil((double)((float)L.h * zr1) / PF_MYPI);
    static const int it3[3] = {200, 100, 50};
    static const int it4[4] = {200, 150, 100, 50};
    L.iters = max_level == 3 ? it3[level] : it4[level];
    return L;
}

TileBox tile_box(const pf_window& r, const LevelDims& L)
{  // Depth.cpp:1497-1562 (enlargement disabled at :1522/:1543; the clamps stay)
    int w = L.w, h = L.h;
    int x0 = (int)round((double)r.az_left / (2 * PF_MYPI) * (double)(w - 1));
    int x1 = (int)round((double)r.az_right / (2 * PF_MYPI) * (double)(w - 1));
    int y0 = (int)round((double)r.zen_top / PF_MYPI * (double)(h - 1));
    int y1 = (int)round((double)r.zen_down / PF_MYPI * (double)(h - 1));
    int xs = x1 >= x0 ? 1 : -1;
    x0 = x0 < 0 ? 0 : (x0 >= w ? w - 1 : x0);
    x1 = x1 < 0 ? 0 : (x1 >= w ? w - 1 : x1);
    y0 = y0 < 0 ? 0 : (y0 >= h ? h - 1 : y0);
    y1 = y1 < 0 ? 0 : (y1 >= h ? h - 1 : y1);
    if (y0 <= L.h0) y0 = L.h0 + 1;
    if (y1 >= L.h1) y1 = L.h1 - 1;
    TileBox b{};
    b.x0 = x0; b.x1 = x1; b.y0 = y0; b.y1 = y1; b.xs = xs;
    return b;
}
}  // namespace

// Fusion grid coordinates (Depth.cpp:1456,1591): az = (float)xx/(float)(w-1)*2*MYPI and
// zen = (float)yy/(float)(h-1)*MYPI, rounded to float by the Vec2f; xx in [-1, w], yy in [-1, h].
void pf::grid_tables(const LevelDims& L, std::vector<GridCol>& cols, std::vector<GridRow>& rows)
{
    cols.resize(L.w + 2);
    rows.resize(L.h + 2);
    for (int xx = -1; xx <= L.w; xx++) {
        float az = (float)((double)((float)xx / (float)(L.w - 1) * 2.0f) * PF_MYPI);
        GridCol c{};
        c.az = az;
        sincosf(az, &c.sa, &c.ca);
        cols[xx + 1] = c;
    }
    for (int yy = -1; yy <= L.h; yy++) {
        float zen = (float)((double)((float)yy / (float)(L.h - 1)) * PF_MYPI);
        GridRow r{};
        r.zen = zen;
        sincosf(zen, &r.sz, &r.cz);
        rows[yy + 1] = r;
    }
}

// ---------------------------------------------------------------------------------------------
extern "C" {

int pf_level_info(int out_w, int out_h, float zr0, float zr1, int level, int* w, int* h,
                  int* h0, int* h1, int* iters, int* nlevels)
{
    if (out_w < 8 || out_h < 4) return PF_EINVAL;
    int nl = out_w >= 4096 ? 4 : 3;
    if (level < 0 || level >= nl) return PF_EINVAL;
    LevelDims L = level_dims(out_w, out_h, zr0, zr1, level);
    if (w) *w = L.w;
    if (h) *h = L.h;
    if (h0) *h0 = L.h0;
    if (h1) *h1 = L.h1;
    if (iters) *iters = L.iters;
    if (nlevels) *nlevels = L.nlevels;
    return PF_OK;
}

int pf_probe_warp_coords(const pf_window* fov, int tile_w, int tile_h, int pw, int ph,
                         uint32_t* wxy, float* wfxy)
{
    if (!fov || !wxy || !wfxy || tile_w < 2 || tile_h < 2 || pw < 2 || ph < 2 || pw >= 65536 ||
        ph >= 65536)
        return PF_EINVAL;
    const TileGeom g = set_window(*fov, tile_w, tile_h, 1);
    warp_coords_host(g, pw, ph, wxy, wfxy);
    return PF_OK;
}

int pf_probe_rgb_taps(const pf_window* fov, int tile_w, int tile_h, int pw, int ph,
                      uint32_t* taps)
{
    static_assert(sizeof(RgbTap) == 16, "RgbTap is 4 words");
    if (!fov || !taps || tile_w < 1 || tile_h < 1 || pw < 2 || ph < 2 || pw >= 65536 ||
        ph >= 65536)
        return PF_EINVAL;
    rgb_taps_host(rgb_cam(*fov), tile_w, tile_h, pw, ph, reinterpret_cast<RgbTap*>(taps));
    return PF_OK;
}

int pf_set_tiles(pf_ctx* c, const pf_window* fovs, const pf_window* ranges, int ntiles,
                 const int* tile_w, const int* tile_h, int tile_c, int cap_ranges)
{
    if (!c) return PF_EINVAL;
    if (!fovs || !ranges || !tile_w || !tile_h || ntiles <= 0 || ntiles > 4096 || tile_c <= 0)
        return fail(c, PF_EINVAL, "pf_set_tiles: bad arguments (ntiles=%d, tile_c=%d)", ntiles,
                    tile_c);
    HIPCHK(c, hipSetDevice(c->device));
    const double cap = 359.9 / 180.0 * PF_MYPI;  // D2R(359.9), MergeDepthMaps :783-784
    {
        // The same layout again (a per-panorama caller such as the DepthNamespace facade):
        // keep the per-layout caches (level boxes, tap maps, registration grids, warp maps).
        bool same = c->layout_ok && c->ntiles == ntiles && c->tile_c == tile_c &&
                    (int)c->tw_h.size() == ntiles && (int)c->th_h.size() == ntiles;
        for (int i = 0; same && i < ntiles; i++) {
            pf_window r = ranges[i];
            if (cap_ranges) {
                r.az_left = (float)((double)r.az_left < cap ? (double)r.az_left : cap);
                r.az_right = (float)((double)r.az_right < cap ? (double)r.az_right : cap);
            }
            same = !memcmp(&c->fov[i], &fovs[i], sizeof(pf_window)) &&
                   !memcmp(&c->rng[i], &r, sizeof(pf_window)) && c->tw_h[i] == tile_w[i] &&
                   c->th_h[i] == tile_h[i];
        }
        if (same) return PF_OK;
    }
    c->layout_ok = false;
    c->ntiles = ntiles;
    c->tile_c = tile_c;
    c->fov.assign(fovs, fovs + ntiles);
    c->rng.assign(ranges, ranges + ntiles);
    c->tw_h.assign(tile_w, tile_w + ntiles);
    c->th_h.assign(tile_h, tile_h + ntiles);
    c->geom_h.resize(ntiles);
    c->reg_h.resize(ntiles);
    std::vector<RgbCam> cams(ntiles);
    std::vector<long long> rgb_off(ntiles);
    long long off = 0, roff = 0, npmax = 0;
    for (int i = 0; i < ntiles; i++) {
        if (tile_w[i] < 2 || tile_h[i] < 2)
            return fail(c, PF_EINVAL, "tile %d: size %dx%d (need >= 2x2)", i, tile_w[i], tile_h[i]);
        pf_window& r = c->rng[i];
        if (cap_ranges) {
            r.az_left = (float)((double)r.az_left < cap ? (double)r.az_left : cap);
            r.az_right = (float)((double)r.az_right < cap ? (double)r.az_right : cap);
        }
        TileGeom g = set_window(fovs[i], tile_w[i], tile_h[i], tile_c);
        if (!(g.hl > 0.0f) || !(g.vl > 0.0f))
            return fail(c, PF_EINVAL, "tile %d: degenerate window (pole or zero FOV)", i);
        g.off = off;
        g.pix_off = (int)(off / tile_c);
        off += (long long)tile_w[i] * tile_h[i] * tile_c;
        if (off / tile_c > INT32_MAX)
            return fail(c, PF_EINVAL, "layout has more than 2^31 tile pixels");
        rgb_off[i] = roff;
        roff += (long long)tile_w[i] * tile_h[i] * 3;
        long long np = (long long)tile_w[i] * tile_h[i];
        if (np > npmax) npmax = np;
        c->geom_h[i] = g;
        cams[i] = rgb_cam(fovs[i]);
    }
    c->tile_elems = off;
    c->rgb_elems = roff;
    c->npix_max = npmax;
    c->lc.out_w = 0;  // boxes and registration grids depend on the ranges: rebuild lazily
    c->reg_valid = false;
    c->st_key[0] = c->st_key[1] = 0;
    c->wmap_pw = c->wmap_ph = 0;
    c->rgb_pw = c->rgb_ph = 0;
    c->cams_h = cams;
    // the ray-factor tables of planar-depth tiles (pf_set_tile_depth): sum (w + h) doubles
    c->ray_h.resize(ntiles);
    c->ray_tab_h.clear();
    for (int i = 0; i < ntiles; i++) {
        const size_t at = c->ray_tab_h.size();
        c->ray_h[i] = RayTile{(int)at, (int)at + tile_w[i]};
        c->ray_tab_h.resize(at + (size_t)tile_w[i] + (size_t)tile_h[i]);
        ray_tables(fovs[i].az_left, fovs[i].az_right, fovs[i].zen_top, fovs[i].zen_down, tile_w[i],
                   tile_h[i], &c->ray_tab_h[at], &c->ray_tab_h[at + tile_w[i]]);
    }
    c->reg_kf_key[0] = -1;
    std::vector<WarpPatch> patches;
    const int pe = warp_patch_edge(), peh = warp_patch_height();
    for (int i = 0; i < ntiles; i++)
        for (int y = 0; y < tile_h[i]; y += peh)
            for (int x = 0; x < tile_w[i]; x += pe) patches.push_back(WarpPatch{i, x, y, 0, 0, 0, 0, 0, 0, 0});
    c->npatch = (int)patches.size();
    c->wpatch_grid_h = patches;
    int rc;
    if ((rc = upload(c, c->wpatch, patches))) return rc;
    if ((rc = upload(c, c->geom, c->geom_h))) return rc;
    if ((rc = upload(c, c->rgb_off, rgb_off))) return rc;
    if ((rc = upload(c, c->ray_tab, c->ray_tab_h))) return rc;
    if ((rc = upload(c, c->ray, c->ray_h))) return rc;
    c->layout_ok = true;
    return PF_OK;
}

int pf_set_tile_depth(pf_ctx* c, int kind)
{
    if (!c) return PF_EINVAL;
    if (kind != PF_TILE_DEPTH_RAY && kind != PF_TILE_DEPTH_PLANAR)
        return fail(c, PF_EINVAL, "pf_set_tile_depth: unknown kind %d", kind);
    c->tile_depth = kind;
    return PF_OK;
}

int pf_tile_ray_tables(pf_ctx* c, int tile, double* cu, double* rv)
{
    if (!c) return PF_EINVAL;
    if (c->ntiles <= 0 || !c->layout_ok)
        return fail(c, PF_ESTATE, "no tile layout: call pf_set_tiles first");
    if (tile < 0 || tile >= c->ntiles || !cu || !rv)
        return fail(c, PF_EINVAL, "pf_tile_ray_tables: bad arguments (tile %d of %d)", tile,
                    c->ntiles);
    const RayTile rt = c->ray_h[tile];
    memcpy(cu, &c->ray_tab_h[rt.cu], sizeof(double) * c->tw_h[tile]);
    memcpy(rv, &c->ray_tab_h[rt.rv], sizeof(double) * c->th_h[tile]);
    return PF_OK;
}

int pf_tile_ray_factor(pf_ctx* c, float* k)
{
    int rc;
    if ((rc = check_common(c, 1))) return rc;
    if (!c->layout_ok) return fail(c, PF_ESTATE, "no tile layout: call pf_set_tiles first");
    if (!k) return fail(c, PF_EINVAL, "pf_tile_ray_factor: k is NULL");
    launch_ray_factor(c->stream, (const TileGeom*)c->geom.p, (const RayTile*)c->ray.p,
                      (const double*)c->ray_tab.p, c->ntiles, c->tile_elems / c->tile_c, k);
    HIPCHK(c, hipGetLastError());
    return PF_OK;
}

int pf_layout_audit(pf_ctx* c, int out_w, int out_h, float zr0, float zr1, int level,
                    pf_level_audit* out)
{
    int rc;
    const LevelDims* Lp = nullptr;
    if ((rc = check_common(c, 1))) return rc;
    if (!out) return fail(c, PF_EINVAL, "NULL buffer");
    if ((rc = level_at(c, out_w, out_h, zr0, zr1, level, &Lp))) return rc;
    const LevelDims& L = *Lp;
    const LevelCache& lc = c->lc;
    const size_t bytes = sizeof(unsigned long long) * kAuditWords;
    if ((rc = ensure(c, c->audit_ws, bytes))) return rc;
    HIPCHK(c, hipMemsetAsync(c->audit_ws.p, 0, bytes, c->stream));
    launch_layout_audit(c->stream, (const TileGeom*)c->geom.p, (const TileBox*)lc.box[level].p,
                        c->ntiles, (const GridCol*)lc.cols[level].p,
                        (const GridRow*)lc.rows[level].p, L, (unsigned long long*)c->audit_ws.p);
    HIPCHK(c, hipGetLastError());
    unsigned long long h[kAuditWords];
    HIPCHK(c, hipMemcpyAsync(h, c->audit_ws.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    out->w = L.w;
    out->h = L.h;
    out->h0 = L.h0;
    out->h1 = L.h1;
    out->taps_outside = (long long)h[0];
    out->taps_clamped = (long long)h[1];
    out->covered = (long long)h[2];
    out->uncovered_interior = (long long)h[3];
    out->max_cover = (int)h[4];
    out->seam = (int)h[5];
    return PF_OK;
}

}  // extern "C"

// Registration tables depend on the zenith range; built per call (tiny, cached by value).
int pf::prepare_registration(pf_ctx* c, float zr0, float zr1)
{
    uint32_t b0, b1;
    memcpy(&b0, &zr0, 4);
    memcpy(&b1, &zr1, 4);
    if (c->reg_valid && b0 == c->reg_zr0 && b1 == c->reg_zr1) return PF_OK;
    const float subd = (float)(1 / 180.0 * PF_MYPI);
    std::vector<GridCol> rcols;
    std::vector<GridRow> rrows;
    int nsamp_total = 0;
    for (int i = 0; i < c->ntiles; i++) {
        const pf_window& r = c->rng[i];
        RegGrid rg{};
        rg.cols = (int)roundf(fabsf(r.az_right - r.az_left) / subd);
        float top = zr0 > r.zen_top ? zr0 : r.zen_top;      // MAX2 (:1301)
        float down = zr1 < r.zen_down ? zr1 : r.zen_down;   // MIN2 (:1302)
        rg.rows = (int)roundf(fabsf(down - top) / subd);
        // an empty grid (the reference divides by 0 there) is an error only for a tile that is
        // solved (check_reg_grids); an inactive tile of a joint solve may have one
        if (rg.cols < 0) rg.cols = 0;
        if (rg.rows < 0) rg.rows = 0;
        rg.col_off = (int)rcols.size();
        rg.row_off = (int)rrows.size();
        rg.soff = nsamp_total;
        for (int k = 0; k <= rg.cols; k++) {  // :1334
            GridCol e{};
            e.az = r.az_left + (r.az_right - r.az_left) * (float)k / (float)rg.cols;
            sincosf(e.az, &e.sa, &e.ca);
            rcols.push_back(e);
        }
        for (int k = 0; k <= rg.rows; k++) {  // :1335
            GridRow e{};
            e.zen = top + (down - top) * (float)k / (float)rg.rows;
            sincosf(e.zen, &e.sz, &e.cz);
            rrows.push_back(e);
        }
        c->reg_h[i] = rg;
        nsamp_total += (rg.cols + 1) * (rg.rows + 1);
    }
    int rc;
    if ((rc = upload(c, c->reg, c->reg_h))) return rc;
    if ((rc = upload(c, c->rcols, rcols))) return rc;
    if ((rc = upload(c, c->rrows, rrows))) return rc;
    c->reg_valid = true;
    c->reg_sidx_key[0] = -1;  // the sample indices follow the grids
    c->reg_kf_key[0] = -1;
    c->pair_valid = false;  // and so does the overlap table
    c->reg_zr0 = b0;
    c->reg_zr1 = b1;
    return PF_OK;
}

// The registration samples' indices for this baseline size (k_regidx), rebuilt when the grids
// or the baseline size change; stream-ordered before the k_register launches that read them.
const int2* pf::reg_sample_index(pf_ctx* c, int ew, int eh, int ec)
{
    if (c->reg_sidx_key[0] == ew && c->reg_sidx_key[1] == eh && c->reg_sidx_key[2] == ec)
        return (const int2*)c->reg_sidx.p;
    long long n = 0;
    int maxn = 0;
    for (const RegGrid& g : c->reg_h) {
        const int k = (g.cols + 1) * (g.rows + 1);
        n += k;
        maxn = k > maxn ? k : maxn;
    }
    if (n <= 0 || ensure(c, c->reg_sidx, sizeof(int2) * (size_t)n) != PF_OK) return nullptr;
    launch_regidx(c->stream, (const TileGeom*)c->geom.p, (const RegGrid*)c->reg.p,
                  (const GridCol*)c->rcols.p, (const GridRow*)c->rrows.p, c->ntiles, maxn, ew,
                  eh, ec, (int2*)c->reg_sidx.p);
    if (hipGetLastError() != hipSuccess) return nullptr;
    c->reg_sidx_key[0] = ew;
    c->reg_sidx_key[1] = eh;
    c->reg_sidx_key[2] = ec;
    return (const int2*)c->reg_sidx.p;
}

// The samples' ray factor (k_reg_kf) for the sample indices of this baseline size; rebuilt when
// they are.  Stream-ordered before the planar registrations that read it.
const float* pf::reg_sample_kf(pf_ctx* c, int ew, int eh, int ec)
{
    const int2* sidx = reg_sample_index(c, ew, eh, ec);
    if (!sidx) return nullptr;
    if (c->reg_kf_key[0] == ew && c->reg_kf_key[1] == eh && c->reg_kf_key[2] == ec)
        return (const float*)c->reg_kf.p;
    long long n = 0;
    int maxn = 0;
    for (const RegGrid& g : c->reg_h) {
        const int k = (g.cols + 1) * (g.rows + 1);
        n += k;
        maxn = k > maxn ? k : maxn;
    }
    if (ensure(c, c->reg_kf, sizeof(float) * (size_t)n) != PF_OK) return nullptr;
    launch_reg_kf(c->stream, (const TileGeom*)c->geom.p, (const RegGrid*)c->reg.p,
                  (const RayTile*)c->ray.p, (const double*)c->ray_tab.p, c->ntiles, maxn, sidx,
                  (float*)c->reg_kf.p);
    if (hipGetLastError() != hipSuccess) return nullptr;
    c->reg_kf_key[0] = ew;
    c->reg_kf_key[1] = eh;
    c->reg_kf_key[2] = ec;
    return (const float*)c->reg_kf.p;
}

// The tiles that will be solved must have a non-empty sample grid (Depth.cpp:1334-1335 divides
// by cols and rows); active == nullptr means every tile.
int pf::check_reg_grids(pf_ctx* c, const int* active)
{
    for (int i = 0; i < c->ntiles; i++) {
        if (active && !active[i]) continue;
        const RegGrid& rg = c->reg_h[i];
        if (rg.cols <= 0 || rg.rows <= 0)
            return fail(c, PF_EINVAL,
                        "tile %d: registration grid %dx%d is empty (the reference divides by 0)",
                        i, rg.cols, rg.rows);
    }
    return PF_OK;
}

int pf::prepare_levels(pf_ctx* c, int out_w, int out_h, float zr0, float zr1)
{
    uint32_t b0, b1;
    memcpy(&b0, &zr0, 4);
    memcpy(&b1, &zr1, 4);
    LevelCache& lc = c->lc;
    if (lc.out_w == out_w && lc.out_h == out_h && lc.zr0 == b0 && lc.zr1 == b1) return PF_OK;
    if (out_w < 8 || out_h < 8)
        return fail(c, PF_EINVAL, "output %dx%d too small", out_w, out_h);
    if ((long long)out_w * out_h >= (1LL << 31))  // per-panorama pixel indices are 32-bit
        return fail(c, PF_EINVAL, "output %dx%d too large", out_w, out_h);
    // the levels are rewritten one by one: invalid until all are (a failed rebuild stays so)
    lc.out_w = 0;
    int nl = out_w >= 4096 ? 4 : 3;
    for (int l = 0; l < nl; l++) {
        LevelDims L = level_dims(out_w, out_h, zr0, zr1, l);
        if (L.w < 4 || L.h < 4 || L.h0 < 1 || L.h1 > L.h - 2 || L.h0 >= L.h1)
            return fail(c, PF_EINVAL,
                        "level %d: %dx%d with band [%d,%d] (zenith range must stay inside "
                        "(0, pi) by a row)",
                        l, L.w, L.h, L.h0, L.h1);
        if (l > 0 && (L.w != 2 * lc.dims[l - 1].w || L.h != 2 * lc.dims[l - 1].h))
            return fail(c, PF_EINVAL, "output %dx%d is not divisible by 2^%d", out_w, out_h,
                        nl - 1);
        lc.dims[l] = L;
        std::vector<TileBox> boxes(c->ntiles);
        std::vector<int> cover((size_t)L.w * L.h, 0);
        for (int p = 0; p < c->ntiles; p++) {
            boxes[p] = tile_box(c->rng[p], L);
            const TileBox& b = boxes[p];
            if (b.x0 == b.x1)
                return fail(c, PF_EDEGENERATE,
                            "tile %d at level %d: box x0 == x1 == %d (the reference never "
                            "terminates here)",
                            p, l, b.x0);
            for (int X = b.x0; X != b.x1; X += b.xs)
                for (int Y = b.y0; Y <= b.y1; Y++)
                    if (++cover[(size_t)Y * L.w + X] > PF_MAX_COVER)
                        return fail(c, PF_EINVAL, "pixel (%d,%d) covered by more than %d tiles",
                                    X, Y, PF_MAX_COVER);
        }
        lc.box_h[l] = boxes;
        {
            std::vector<int2> mc;
            for (size_t o = 0; o < cover.size(); o++) {
                if (cover[o] <= 2) continue;
                const int Y = (int)(o / L.w), X = (int)(o % L.w);
                for (int p = 0; p < c->ntiles; p++) {
                    const TileBox& b = boxes[p];
                    const bool in = Y >= b.y0 && Y <= b.y1 &&
                                    (b.xs > 0 ? (X >= b.x0 && X < b.x1) : (X <= b.x0 && X > b.x1));
                    if (in) mc.push_back(make_int2((int)o, p));
                }
            }
            lc.nmc[l] = (int)mc.size();
            int rc2;
            if ((rc2 = upload(c, lc.mcpairs[l], mc))) return rc2;
        }
        std::vector<float> hcol(L.w, 0.0f);
        bool full = L.h0 + 1 < L.h1;
        for (int X = 0; X < L.w && full; X++)
            hcol[X] = cover[(size_t)(L.h0 + 1) * L.w + X] > 0 ? 0.5f : 0.0f;
        full = full && hcol[0] == 0.0f;
        for (int Y = L.h0; Y <= L.h1 && full; Y++)
            for (int X = 0; X < L.w; X++)
                if ((cover[(size_t)Y * L.w + X] > 0) != (hcol[X] != 0.0f && Y > L.h0 && Y < L.h1)) {
                    full = false;
                    break;
                }
        lc.full[l] = full;
        std::vector<GridCol> cols;
        std::vector<GridRow> rows;
        grid_tables(L, cols, rows);
        int rc;
        {   // per targets patch of this level, mask words of the tiles whose box meets it (the
            // device's box_meets on the patch rectangle targets_patch uses)
            const int pw_ = targets_patch_w(), ph_ = targets_patch_h();
            const int npx = (L.w + pw_ - 1) / pw_, npy = (L.h1 - L.h0 + 1 + ph_ - 1) / ph_;
            const int nmw = (c->ntiles + 31) / 32;
            std::vector<uint32_t> tm((size_t)npx * npy * nmw, 0u);
            for (int pid = 0; pid < npx * npy; pid++) {
                const int X0 = (pid % npx) * pw_, Y0 = L.h0 + (pid / npx) * ph_;
                const int X1 = std::min(X0 + pw_ - 1, L.w - 1), Y1 = std::min(Y0 + ph_ - 1, L.h1);
                for (int p = 0; p < c->ntiles; p++)
                    if (box_meets(boxes[p], X0, X1, Y0, Y1))
                        tm[(size_t)pid * nmw + p / 32] |= 1u << (p % 32);
            }
            if ((rc = upload(c, lc.tmask[l], tm))) return rc;
        }
        if ((rc = upload(c, lc.box[l], boxes))) return rc;
        if ((rc = upload(c, lc.hcol[l], hcol))) return rc;
        if ((rc = upload(c, lc.cols[l], cols))) return rc;
        if ((rc = upload(c, lc.rows[l], rows))) return rc;
        // tap-index maps: every tile's box plus a one-pixel ring (pf_targets.hip)
        std::vector<TapBox> tbs(c->ntiles);
        long long moff = 0, maxpts = 0;
        for (int p = 0; p < c->ntiles; p++) {
            const TileBox& b = boxes[p];
            TapBox t{};
            if (b.y0 <= b.y1) {
                int xlo = b.xs > 0 ? b.x0 : b.x1 + 1, xhi = b.xs > 0 ? b.x1 - 1 : b.x0;
                t.xmin = xlo - 1;
                t.ymin = b.y0 - 1;
                t.nx = xhi - xlo + 3;
                t.ny = b.y1 - b.y0 + 3;
            }
            t.off = moff;
            long long np = (long long)t.nx * t.ny;
            moff += np;
            if (np > maxpts) maxpts = np;
            tbs[p] = t;
        }
        if ((rc = upload(c, lc.tapbox[l], tbs))) return rc;
        if ((rc = ensure(c, lc.tapmap[l], sizeof(int32_t) * (moff + 1)))) return rc;
        lc.taps[l] = moff;
        launch_tapmap(c->stream, (const TileGeom*)c->geom.p, (const TapBox*)lc.tapbox[l].p,
                      c->ntiles, maxpts, (const GridCol*)lc.cols[l].p,
                      (const GridRow*)lc.rows[l].p, (int32_t*)lc.tapmap[l].p);
        HIPCHK(c, hipGetLastError());
    }
    {
        // gather order of k_targets_multi: zenith bands = the coarsest level's patch rows; per
        // band the finest level's patches first, then each coarser level's patches of that band
        const int pw_ = targets_patch_w(), ph_ = targets_patch_h();
        int npy[4], npx[4];
        for (int l = 0; l < nl; l++) {
            npx[l] = (lc.dims[l].w + pw_ - 1) / pw_;
            npy[l] = (lc.dims[l].h1 - lc.dims[l].h0 + 1 + ph_ - 1) / ph_;
        }
        std::vector<int2> order;
        for (int j = 0; j < npy[0]; j++)
            for (int l = nl - 1; l >= 0; l--)
                for (int r = 0; r < npy[l]; r++) {
                    const int band = std::min(npy[0] - 1, (int)((long long)r * npy[0] / npy[l]));
                    if (band != j) continue;
                    for (int x = 0; x < npx[l]; x++) order.push_back(make_int2(l, r * npx[l] + x));
                }
        int rc;
        if ((rc = upload(c, lc.tgt_order, order))) return rc;
        lc.tgt_nentries = (int)order.size();
    }
    lc.nlevels = nl;
    lc.out_w = out_w;
    lc.out_h = out_h;
    lc.zr0 = b0;
    lc.zr1 = b1;
    return PF_OK;
}
