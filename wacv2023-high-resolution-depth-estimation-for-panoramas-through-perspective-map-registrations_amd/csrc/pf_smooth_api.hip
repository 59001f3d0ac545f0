// pf_smooth_api.hip -- pf_solve_smoothing: SolveDepthBySmoothing's host-side list building and
// launch sequence.
#include "pf_ctx.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>

using namespace pf;

extern "C" {

int pf_solve_smoothing(pf_ctx* c, const float* tiles, const float* coeffs, int batch, int out_w,
                       int out_h, float zr0, float zr1, uint16_t* out)
{  // SolveDepthBySmoothing (Depth.cpp:1773-1878)
    int rc;
    if ((rc = check_common(c, batch))) return rc;
    if ((rc = check_unmasked(c, "pf_solve_smoothing"))) return rc;
    if ((rc = check_ray_coeffs(c, "pf_solve_smoothing", coeffs))) return rc;
    if ((rc = jres_check(c))) return rc;  // an earlier call's timeout, once it has landed
    if (!tiles || !out) return fail(c, PF_EINVAL, "tiles/out is NULL");
    if (out_w < 3 || out_h < 3 || (long long)out_w * out_h >= (1LL << 31))
        return fail(c, PF_EINVAL, "output %dx%d out of range", out_w, out_h);
    LevelDims L{};
    L.w = out_w;
    L.h = out_h;
    L.h0 = (int)floor((double)((float)out_h * zr0) / PF_MYPI);  // height0/height1 (:1781-1782)
    L.h1 = (int)ceil((double)((float)out_h * zr1) / PF_MYPI);
    if (L.h0 < 1 || L.h1 > out_h - 2 || L.h0 > L.h1)
        return fail(c, PF_EINVAL, "rows [%d, %d] of %d: the smoothing stencil would leave the "
                    "buffer (the reference reads out of bounds)", L.h0, L.h1, out_h);
    std::vector<SmoothBox> boxes(c->ntiles);
    for (int p = 0; p < c->ntiles; p++) {  // :1795-1805, no clamps
        const pf_window& r = c->rng[p];
        SmoothBox b{};
        b.x0 = (int)round((double)r.az_left / (2 * PF_MYPI) * (double)(out_w - 1));
        b.x1 = (int)round((double)r.az_right / (2 * PF_MYPI) * (double)(out_w - 1));
        b.y0 = (int)round((double)r.zen_top / PF_MYPI * (double)(out_h - 1));
        b.y1 = (int)round((double)r.zen_down / PF_MYPI * (double)(out_h - 1));
        b.xs = b.x1 >= b.x0 ? 1 : -1;
        if (b.x0 == b.x1)
            return fail(c, PF_EDEGENERATE, "tile %d: box x0 == x1 == %d (the reference never "
                        "terminates here)", p, b.x0);
        if (b.x0 < 0 || b.x0 >= out_w || b.x1 < 0 || b.x1 >= out_w || b.y0 < 0 || b.y1 >= out_h)
            return fail(c, PF_EINVAL, "tile %d: box (%d..%d, %d..%d) leaves the %dx%d output (the "
                        "reference writes out of bounds)", p, b.x0, b.x1, b.y0, b.y1, out_w, out_h);
        boxes[p] = b;
    }
    std::vector<GridCol> cols;
    std::vector<GridRow> rows;
    grid_tables(L, cols, rows);
    const long long n = (long long)out_w * out_h;
    if ((rc = upload(c, c->sm_box, boxes))) return rc;
    if ((rc = upload(c, c->sm_cols, cols))) return rc;
    if ((rc = upload(c, c->sm_rows, rows))) return rc;
    if ((rc = ensure(c, c->sm_src, sizeof(int2) * n))) return rc;
    if ((rc = ensure(c, c->sm_mask, n))) return rc;
    if ((rc = ensure(c, c->buf[0], sizeof(float) * n * batch))) return rc;
    launch_smooth_map(c->stream, (const TileGeom*)c->geom.p, (const SmoothBox*)c->sm_box.p,
                      c->ntiles, (const GridCol*)c->sm_cols.p, (const GridRow*)c->sm_rows.p,
                      out_w, out_h, (int2*)c->sm_src.p, (uint8_t*)c->sm_mask.p);
    const int iters = 500;  // :1838
    static const bool scan = getenv("PF_SMOOTH_SCAN") && atoi(getenv("PF_SMOOTH_SCAN"));
    if (scan) {  // every (X, Y) of the diagonal tested against the mask (the first form)
        launch_smooth(c->stream, (const TileGeom*)c->geom.p, c->ntiles, (const int2*)c->sm_src.p,
                      (const uint8_t*)c->sm_mask.p, tiles, c->tile_elems, coeffs, out_w, out_h,
                      L.h0, L.h1, iters, (float*)c->buf[0].p, batch);
    } else {
        // row blocks per panorama (k_smooth_band): a panorama's steps spread over nb CUs;
        // PF_SMOOTH_BAND=0 keeps one workgroup per panorama (k_smooth_iter_list, nb = 1)
        const char* be = getenv("PF_SMOOTH_BAND");  // read per call (tests vary it)
        const int band_mode = be ? atoi(be) : 1;
        int nb = 1;
        if (band_mode != 0) {
            nb = band_mode > 1 ? band_mode : std::max(1, std::min(64, 1024 / batch));
            nb = std::max(1, std::min(nb, (L.h1 - L.h0 + 1) / 4));
        }
        const bool same = c->sm_key_boxes.size() == boxes.size() && c->sm_key[0] == out_w &&
                          c->sm_key[1] == out_h && c->sm_key[2] == L.h0 && c->sm_key[3] == L.h1 &&
                          c->sm_nb == nb &&
                          std::equal(boxes.begin(), boxes.end(), c->sm_key_boxes.begin(),
                                     [](const SmoothBox& a, const SmoothBox& b) {
                                         return a.x0 == b.x0 && a.x1 == b.x1 && a.y0 == b.y0 &&
                                                a.y1 == b.y1 && a.xs == b.xs;
                                     });
        if (!same) {  // per row block, the masked pixels by parity of d = X + Y, sorted by d
            std::vector<uint8_t> mask(n);
            HIPCHK(c, hipMemcpyAsync(mask.data(), c->sm_mask.p, n, hipMemcpyDeviceToHost,
                                     c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            const int nk = (out_w + out_h) / 2 + 1;  // d = 2k + p < w + h
            // row blocks of about equal masked-pixel counts
            std::vector<long long> rowcnt(out_h, 0);
            long long total = 0;
            for (int Y = L.h0; Y <= L.h1; Y++) {
                for (int X = 1; X <= out_w - 2; X++) rowcnt[Y] += mask[(long long)Y * out_w + X];
                total += rowcnt[Y];
            }
            std::vector<int> blk_of(out_h, 0);
            {
                long long acc = 0;
                int b = 0, rows_in = 0;
                for (int Y = L.h0; Y <= L.h1; Y++) {
                    const int rows_left = L.h1 - Y + 1;
                    if (b < nb - 1 && rows_in > 0 &&
                        (acc >= total * (b + 1) / nb || rows_left <= nb - 1 - b)) {
                        b++;
                        rows_in = 0;
                    }
                    blk_of[Y] = b;
                    acc += rowcnt[Y];
                    rows_in++;
                }
            }
            const size_t per = (size_t)(nk + 1);
            std::vector<int> cnt((size_t)nb * 2 * per, 0);
            int dmin = INT32_MAX, dmax = -1;
            for (int Y = L.h0; Y <= L.h1; Y++)
                for (int X = 1; X <= out_w - 2; X++)
                    if (mask[(long long)Y * out_w + X]) {
                        const int d = X + Y;
                        cnt[((size_t)blk_of[Y] * 2 + (d & 1)) * per + (d >> 1) + 1]++;
                        dmin = std::min(dmin, d);
                        dmax = std::max(dmax, d);
                    }
            std::vector<int> off(cnt.size());
            int acc = 0;
            for (size_t q = 0; q < (size_t)nb * 2; q++)
                for (size_t k = 0; k < per; k++) {
                    acc += cnt[q * per + k];
                    off[q * per + k] = acc;  // k = 0 holds the zero count: start of d = p
                }
            std::vector<int> fill(off), list(std::max(acc, 1));
            for (int Y = L.h0; Y <= L.h1; Y++)
                for (int X = 1; X <= out_w - 2; X++)
                    if (mask[(long long)Y * out_w + X]) {
                        const int d = X + Y;
                        list[fill[((size_t)blk_of[Y] * 2 + (d & 1)) * per + (d >> 1)]++] =
                            Y * out_w + X;
                    }
            if ((rc = upload(c, c->sm_list, list))) return rc;
            if ((rc = upload(c, c->sm_off, off))) return rc;
            c->sm_nk = nk;
            c->sm_nb = nb;
            c->sm_smin = dmin;
            c->sm_smax = dmax < 0 ? -1 : dmax + 2 * (iters - 1);
            c->sm_key_boxes = boxes;
            c->sm_key[0] = out_w; c->sm_key[1] = out_h; c->sm_key[2] = L.h0; c->sm_key[3] = L.h1;
        }
        launch_smooth_seed(c->stream, (const TileGeom*)c->geom.p, c->ntiles,
                           (const int2*)c->sm_src.p, tiles, c->tile_elems, coeffs, out_w, out_h,
                           (float*)c->buf[0].p, batch);
        if (c->sm_smax >= c->sm_smin) {
            if (nb == 1) {
                launch_smooth_list(c->stream, (const int*)c->sm_list.p, (const int*)c->sm_off.p,
                                   c->sm_nk, out_w, out_h, c->sm_smin, c->sm_smax, iters,
                                   (float*)c->buf[0].p, batch);
            } else {
                // sync words: [0] ticket, [1] timeouts, [2..] one step flag per (panorama, block);
                // tickets and flags are monotone across launches (sm_tk, sm_fb)
                const size_t sb = sizeof(uint32_t) * (2 + (size_t)batch * nb);
                if (c->sm_sync.bytes < sb) {
                    if ((rc = ensure(c, c->sm_sync, sb))) return rc;
                    HIPCHK(c, hipMemsetAsync(c->sm_sync.p, 0, sb, c->stream));
                    c->sm_tk = 0;
                    c->sm_fb = 1;
                }
                if ((rc = ensure_err_host(c))) return rc;
                SmoothSync S{};
                uint32_t* w32 = (uint32_t*)c->sm_sync.p;
                S.ticket = w32;
                S.err = w32 + 1;
                S.flags = w32 + 2;
                S.err_host = c->jres_err_h;
                S.tbase = c->sm_tk;
                S.fbase = c->sm_fb;
                S.spin_log2 = 22;
                if (c->smooth_fault) {  // pf_debug_smooth_fault: this launch only
                    S.fault = 1;
                    S.spin_log2 = c->smooth_fault;
                    c->smooth_fault = 0;
                }
                c->sm_tk += (uint32_t)(batch * nb);
                c->sm_fb += (uint32_t)(c->sm_smax - c->sm_smin + 2);
                launch_smooth_band(c->stream, (const int*)c->sm_list.p, (const int*)c->sm_off.p,
                                   c->sm_nk, nb, out_w, out_h, c->sm_smin, c->sm_smax, iters,
                                   (float*)c->buf[0].p, batch, S);
            }
        }
    }
    launch_quantize(c->stream, (const float*)c->buf[0].p, n, (int)n, out, n, batch);
    HIPCHK(c, hipGetLastError());
    return PF_OK;
}

}  // extern "C"
