// pf_warp_api.hip -- pf_warp_depth / pf_warp_rgb: the per-(layout, panorama size) warp tables,
// built on the host on first use, and the warp launches.
#include "pf_ctx.hpp"

#include <algorithm>
#include <cstdlib>
#include <numeric>

using namespace pf;

// The per-pixel warp tables are built on the host (glibc atan2f: the reference's bits), tiles
// packed into one host staging run of up to 2^24 pixels (C3's whole layout; C5 in 6 runs) that is
// uploaded with one copy per array and one synchronisation per run.  That first call per panorama
// size blocks the host (the staging memory is reused).
static size_t stage_capacity(const pf_ctx* c, long long npix)
{
    const size_t kStagePix = (size_t)1 << 24;
    return std::max((size_t)c->npix_max, std::min((size_t)npix, kStagePix));
}

// Packs tiles p0.. into a staging run of at most cap pixels (one tile at least): build(p, g, at)
// fills tile p's tables at pixel offset `at` of the run.  Returns the first tile after the run,
// *n = the run's pixels.
template <class Build>
static int stage_run(const pf_ctx* c, int p0, size_t cap, size_t* n, Build build)
{
    *n = 0;
    int p1 = p0;
    for (; p1 < c->ntiles; p1++) {
        const TileGeom& g = c->geom_h[p1];
        const size_t m = (size_t)g.w * g.h;
        if (p1 > p0 && *n + m > cap) break;
        build(p1, g, *n);
        *n += m;
    }
    return p1;
}

// The stable order of items 0..n-1 by key(q).  Both warps order their patches by panorama
// footprint -- 32-row bands, then azimuth -- instead of tile by tile: the blocks resident on one
// XCD then stage overlapping footprints (neighbouring patches of a tile and the overlapping
// patches of the neighbouring tiles) at about the same time, so a panorama line is fetched from
// HBM once and re-read from that XCD's L2 instead of once per box that holds it (the boxes hold
// each panorama pixel ~3 times at the C2 layout).  Patches are self-describing, so the
// permutation is free.
template <class Key>
static std::vector<size_t> stable_order(size_t n, Key key)
{
    std::vector<long long> keys(n);
    for (size_t q = 0; q < n; q++) keys[q] = key(q);
    std::vector<size_t> ord(n);
    std::iota(ord.begin(), ord.end(), (size_t)0);
    std::stable_sort(ord.begin(), ord.end(), [&](size_t a, size_t b) { return keys[a] < keys[b]; });
    return ord;
}

// Once per (layout, panorama size), for the bounding boxes k_patch_box wrote: footprint order by
// the box centre.
static int sort_warp_patches(pf_ctx* c, int pw)
{
    std::vector<WarpPatch> p(c->npatch);
    HIPCHK(c, hipMemcpyAsync(p.data(), c->wpatch.p, sizeof(WarpPatch) * p.size(),
                             hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const std::vector<size_t> ord = stable_order(p.size(), [&](size_t q) {
        const WarpPatch& w = p[q];
        const long long band = (w.gy0 + w.bh / 2) / 32;
        const long long col = (w.gx0 + w.bw / 2) % pw;
        return band * 65536 + col;
    });
    std::vector<WarpPatch> sp(p.size());
    for (size_t q = 0; q < ord.size(); q++) sp[q] = p[ord[q]];
    return upload(c, c->wpatch, sp);
}

extern "C" {

int pf_warp_depth(pf_ctx* c, const float* pano, int pw, int ph, int batch,
                  const pf_response* resp, float* tiles)
{
    int rc;
    if ((rc = check_common(c, batch))) return rc;
    if (!pano || !tiles || pw < 2 || ph < 2)
        return fail(c, PF_EINVAL, "bad pano %p %dx%d", (const void*)pano, pw, ph);
    static_assert(sizeof(pf_response) == sizeof(Resp), "pf_response layout");
    if ((long long)pw * ph >= (1ll << 30) || pw >= 65536 || ph >= 65536)
        return fail(c, PF_EINVAL, "pano %dx%d: too large (< 2^30 pixels, sides < 65536)", pw, ph);
    if (c->tile_elems >= (1ll << 29))  // the warp addresses a panorama's tile block with 32-bit
        return fail(c, PF_EINVAL, "tile block of %lld floats: too large for the depth warp "
                    "(< 2^29)", c->tile_elems);      // byte offsets (buffer stores)
    const long long npix = c->tile_elems / c->tile_c;
    if (c->wmap_pw != pw || c->wmap_ph != ph) {
        if ((rc = ensure(c, c->wmap, sizeof(uint32_t) * npix))) return rc;
        if ((rc = ensure(c, c->wfxy, sizeof(float) * 2 * npix))) return rc;
        const size_t cap = stage_capacity(c, npix);
        std::vector<uint32_t> wxy(cap), loc;
        std::vector<float> wf(2 * cap);
        // ragged footprints (host, warp_patches_host: 16-B units) when pw % 4 == 0; else the
        // bounding boxes of k_patch_box / k_warp_local
        const bool ragged = (pw % 4) == 0;
        std::vector<WarpPatch> patches;
        std::vector<uint32_t> units;
        if (ragged) loc.resize(cap);
        for (int p0 = 0; p0 < c->ntiles;) {
            const size_t off0 = (size_t)c->geom_h[p0].pix_off;
            size_t n = 0;
            p0 = stage_run(c, p0, cap, &n, [&](int p, const TileGeom& g, size_t at) {
                warp_coords_host(g, pw, ph, wxy.data() + at, wf.data() + 2 * at);
                if (ragged)
                    warp_patches_host(g, p, wxy.data() + at, pw, ph, patches, units,
                                      loc.data() + at);
            });
            HIPCHK(c, hipMemcpyAsync((uint32_t*)c->wmap.p + off0, ragged ? loc.data() : wxy.data(),
                                     4 * n, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync((float*)c->wfxy.p + 2 * off0, wf.data(), 8 * n,
                                     hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));  // the staging run is reused
        }
        if (ragged) {
            // footprint order, as sort_warp_patches: 32-row bands of the first staged unit, then
            // its column (a wide patch: its first corner)
            const std::vector<size_t> ord = stable_order(patches.size(), [&](size_t q) {
                const WarpPatch& P = patches[q];
                long long row, col;
                if (P.units > 0) {
                    const uint32_t e = units[P.uoff] / 4u;
                    row = e / (uint32_t)pw;
                    col = e % (uint32_t)pw;
                } else {
                    const TileGeom& g = c->geom_h[P.tile];
                    row = 0;
                    col = P.X0 + (long long)g.w * P.Y0;  // keep tile order among wide patches
                }
                return (row / 32) * (1LL << 40) + col;
            });
            std::vector<WarpPatch> sp(patches.size());
            for (size_t q = 0; q < ord.size(); q++) sp[q] = patches[ord[q]];
            if (units.empty()) units.push_back(0u);
            if ((rc = upload(c, c->wpatch, sp))) return rc;
            if ((rc = upload(c, c->wunits, units))) return rc;
            c->npatch = (int)sp.size();
        } else {
            // the plain patch grid (a ragged build for another size replaced it)
            if ((rc = upload(c, c->wpatch, c->wpatch_grid_h))) return rc;
            c->npatch = (int)c->wpatch_grid_h.size();
            launch_warp_boxes(c->stream, (const TileGeom*)c->geom.p, (WarpPatch*)c->wpatch.p,
                              c->npatch, pw, ph, (uint32_t*)c->wmap.p);
            HIPCHK(c, hipGetLastError());
            if ((rc = sort_warp_patches(c, pw))) return rc;
        }
        c->wmap_pw = pw;
        c->wmap_ph = ph;
    }
    StageTimer t(c, PF_STAGE_WARP, batch * (4.0 * pw * ph + 4.0 * (double)npix), 1);
    launch_warp_depth(c->stream, (const TileGeom*)c->geom.p, c->ntiles,
                      (const WarpPatch*)c->wpatch.p, (const uint32_t*)c->wunits.p, c->npatch,
                      (const uint32_t*)c->wmap.p,
                      (const float*)c->wfxy.p, pano, pw, ph, (long long)pw * ph,
                      (const Resp*)resp, tiles, c->tile_elems, batch);
    HIPCHK(c, hipGetLastError());
    return PF_OK;
}

int pf_warp_rgb(pf_ctx* c, const uint8_t* pano, int pw, int ph, int batch, uint8_t* tiles)
{
    int rc;
    if ((rc = check_common(c, batch))) return rc;
    if (!pano || !tiles || pw < 2 || ph < 2)
        return fail(c, PF_EINVAL, "bad pano %p %dx%d", (const void*)pano, pw, ph);
    if (pw >= 65536 || ph >= 65536)
        return fail(c, PF_EINVAL, "pano %dx%d: sides must be < 65536", pw, ph);
    if (c->rgb_pw != pw || c->rgb_ph != ph) {  // the taps of this size, on the host (glibc)
        const long long npix = c->tile_elems / c->tile_c;
        if ((rc = ensure(c, c->rgbtap, sizeof(RgbTap) * npix))) return rc;
        // the LDS-staged kernel needs 16-B units that never straddle the row wrap, 12-B
        // stores of 4 whole pixels, and 32-bit byte offsets (else the per-pixel kernel runs)
        const bool naive = getenv("PF_WARP_RGB_NAIVE") && atoi(getenv("PF_WARP_RGB_NAIVE"));
        bool staged = !naive && (3 * pw) % 16 == 0 && 3LL * pw * ph < (1LL << 31) &&
                      c->rgb_elems < (1LL << 31);
        for (int p = 0; staged && p < c->ntiles; p++) staged = c->geom_h[p].w % 4 == 0;
        if (staged) {
            if ((rc = ensure(c, c->rgbloc, sizeof(uint32_t) * npix))) return rc;
            if ((rc = ensure(c, c->rgbw, sizeof(float) * 2 * npix))) return rc;
        }
        const size_t cap = stage_capacity(c, npix);
        std::vector<RgbTap> taps(cap);
        std::vector<uint32_t> loc(staged ? cap : 0);
        std::vector<float> wts(staged ? 2 * cap : 0);
        std::vector<RgbPatch> patches;
        std::vector<uint32_t> units;
        for (int p0 = 0; p0 < c->ntiles;) {
            const size_t off0 = (size_t)c->geom_h[p0].pix_off;
            size_t n = 0;
            p0 = stage_run(c, p0, cap, &n, [&](int p, const TileGeom& g, size_t at) {
                rgb_taps_host(c->cams_h[p], g.w, g.h, pw, ph, taps.data() + at);
                if (staged)
                    rgb_patches_host(g, p, taps.data() + at, pw, ph, patches, units,
                                     loc.data() + at, wts.data() + 2 * at);
            });
            HIPCHK(c, hipMemcpyAsync((RgbTap*)c->rgbtap.p + off0, taps.data(),
                                     sizeof(RgbTap) * n, hipMemcpyHostToDevice, c->stream));
            if (staged) {
                HIPCHK(c, hipMemcpyAsync((uint32_t*)c->rgbloc.p + off0, loc.data(), 4 * n,
                                         hipMemcpyHostToDevice, c->stream));
                HIPCHK(c, hipMemcpyAsync((float*)c->rgbw.p + 2 * off0, wts.data(), 8 * n,
                                         hipMemcpyHostToDevice, c->stream));
            }
            HIPCHK(c, hipStreamSynchronize(c->stream));  // the staging run is reused
        }
        if (staged) {
            // footprint order (32-row bands of the first staged unit, then azimuth), as the
            // depth warp's patches.  Each patch carries its unit-table row along.
            const uint32_t rowb = (uint32_t)(3 * pw);
            const std::vector<size_t> ord = stable_order(patches.size(), [&](size_t q) {
                const uint32_t u = units[q * kRgbUnits];
                return (long long)(u / rowb / 32) * 65536 + (u % rowb) / 3;
            });
            std::vector<RgbPatch> sp(patches.size());
            std::vector<uint32_t> su(units.size());
            for (size_t q = 0; q < ord.size(); q++) {
                sp[q] = patches[ord[q]];
                std::copy(units.begin() + ord[q] * kRgbUnits,
                          units.begin() + (ord[q] + 1) * kRgbUnits, su.begin() + q * kRgbUnits);
            }
            if ((rc = upload(c, c->rgbpatch, sp))) return rc;
            if ((rc = upload(c, c->rgbunits, su))) return rc;
            c->n_rgbpatch = (int)patches.size();
        }
        c->rgb_staged = staged;
        c->rgb_pw = pw;
        c->rgb_ph = ph;
    }
    StageTimer t(c, PF_STAGE_WARP, batch * (3.0 * pw * ph + (double)c->rgb_elems), 1);
    if (c->rgb_staged)
        launch_warp_rgb_box(c->stream, (const TileGeom*)c->geom.p, (const RgbPatch*)c->rgbpatch.p,
                            c->n_rgbpatch, (const uint32_t*)c->rgbunits.p,
                            (const uint32_t*)c->rgbloc.p, (const float*)c->rgbw.p,
                            (const RgbTap*)c->rgbtap.p, (const long long*)c->rgb_off.p, pano, pw,
                            ph, (long long)pw * ph * 3, tiles, c->rgb_elems, batch);
    else
        launch_warp_rgb(c->stream, (const RgbTap*)c->rgbtap.p, (const TileGeom*)c->geom.p,
                        c->ntiles, c->npix_max, (const long long*)c->rgb_off.p, pano, pw, ph,
                        (long long)pw * ph * 3, tiles, c->rgb_elems, batch);
    HIPCHK(c, hipGetLastError());
    return PF_OK;
}

}  // extern "C"
