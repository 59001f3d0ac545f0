// pf_eval.hip -- the evaluation entry points: ErrorData / ErrorEmap, ErrorLaplacian, ErrorCompare
// and the two in-place depth maps.
#include "pf_ctx.hpp"

#include <algorithm>

using namespace pf;

extern "C" {

int pf_set_metrics_order(pf_ctx* c, int order)
{
    if (!c) return PF_EINVAL;
    if (order != PF_METRICS_SEQUENTIAL && order != PF_METRICS_TREE)
        return fail(c, PF_EINVAL, "metrics order %d", order);
    c->metrics_order = order;
    return PF_OK;
}

int pf_error_metrics(pf_ctx* c, const float* gt, int gw, int gh, int gc, const float* given,
                     const uint16_t* given16, int w, int h, int given_c, int batch, float zr0,
                     float zr1, int align_way, int cap_depth, pf_metrics* out)
{
    int rc;
    if ((rc = check_device(c))) return rc;
    if (!gt || !out || (!given == !given16))
        return fail(c, PF_EINVAL, "pf_error_metrics: need gt, out and exactly one of given/given16");
    if (gw < 1 || gh < 1 || gc < 1 || w < 1 || h < 1 || (given && given_c < 1))
        return fail(c, PF_EINVAL, "pf_error_metrics: bad shape gt %dx%dx%d given %dx%dx%d", gw,
                    gh, gc, w, h, given_c);
    if (batch <= 0 || batch > 65535) return fail(c, PF_EINVAL, "batch %d out of range", batch);
    if (align_way < 0 || align_way > 2) return fail(c, PF_EINVAL, "align_way %d", align_way);
    if ((long long)w * h >= (1ll << 31) || (long long)gw * gh * gc >= (1ll << 31))
        return fail(c, PF_EINVAL, "pf_error_metrics: map too large");
    // Depth.cpp:1984-1985 (int)(g_zenith_range[k] / MYPI * data_height), fp64
    MetricsJob j;
    j.gt = gt;
    j.gw = gw;
    j.gh = gh;
    j.gc = gc;
    j.given = given;
    j.given16 = given16;
    j.w = w;
    j.h = h;
    j.gc_given = given16 ? 1 : given_c;
    j.batch = batch;
    j.h0 = std::max(0, (int)((double)zr0 / PF_MYPI * h));
    j.h1 = std::min(h - 1, (int)((double)zr1 / PF_MYPI * h));
    if (j.h1 < j.h0) return fail(c, PF_EINVAL, "pf_error_metrics: empty zenith band");
    j.align_way = align_way;
    j.cap_depth = cap_depth ? 1 : 0;
    j.sequential = c->metrics_order == PF_METRICS_SEQUENTIAL ? 1 : 0;
    if ((rc = ensure(c, c->metrics_ws, metrics_workspace_bytes(j)))) return rc;
    // algorithmic bytes: one read of the compared band of gt (4 B, channel 0) and of the
    // result (2 B u16 / 4 B f32); the kernels make 4 passes (3 radix digits + the sums) for
    // align_way 1, 2 for align_way 2, 1 otherwise
    const double band = (double)(j.h1 - j.h0 + 1) * w;
    const int passes = align_way == 1 ? 4 : (align_way == 2 ? 2 : 1);
    StageTimer t(c, PF_STAGE_METRICS, batch * band * (4.0 + (given16 ? 2.0 : 4.0)),
                 align_way == 1 ? 9 : passes + 2);
    launch_metrics(c->stream, j, c->metrics_ws.p, out);
    HIPCHK(c, hipGetLastError());
    return PF_OK;
}

int pf_error_laplacian(pf_ctx* c, const float* gt, int gw, int gh, int gc, const float* given,
                       const uint16_t* given16, int w, int h, int given_c, int batch,
                       pf_edge_metrics* out, double* gt_lap, double* given_lap, double* lap_ae)
{
    int rc;
    if ((rc = check_device(c))) return rc;
    if (!gt || !out || (!given == !given16))
        return fail(c, PF_EINVAL,
                    "pf_error_laplacian: need gt, out and exactly one of given/given16");
    if (gw < 1 || gh < 1 || gc < 1 || w < 1 || h < 1 || (given && given_c < 1))
        return fail(c, PF_EINVAL, "pf_error_laplacian: bad shape gt %dx%dx%d given %dx%dx%d", gw,
                    gh, gc, w, h, given_c);
    if (batch <= 0 || batch > 65535) return fail(c, PF_EINVAL, "batch %d out of range", batch);
    if ((long long)w * h >= (1ll << 31) || (long long)gw * gh * gc >= (1ll << 31) ||
        (given && (long long)w * h * given_c >= (1ll << 31)))
        return fail(c, PF_EINVAL, "pf_error_laplacian: map too large");
    EdgeJob j;
    j.gt = gt;
    j.gw = gw;
    j.gh = gh;
    j.gc = gc;
    j.given = given;
    j.given16 = given16;
    j.w = w;
    j.h = h;
    j.gc_given = given16 ? 1 : given_c;
    j.batch = batch;
    j.gt_lap = gt_lap;
    j.given_lap = given_lap;
    j.lap_ae = lap_ae;
    const long long rows = ((long long)h + EDGE_TILE_Y - 1) / EDGE_TILE_Y;
    const long long cols = ((long long)w + EDGE_TILE_X - 1) / EDGE_TILE_X;
    if (rows > 65535 || rows * cols * batch >= (1ll << 31))
        return fail(c, PF_EINVAL, "pf_error_laplacian: %dx%d x %d panoramas: too many tiles", w, h,
                    batch);
    if ((rc = ensure(c, c->metrics_ws, edge_workspace_bytes(j)))) return rc;
    // algorithmic bytes: one read of gt (4 B, channel 0) and of the given map (2 B u16 / 4 B
    // f32), plus 8 B per pixel for each requested plane
    const int planes = (gt_lap ? 1 : 0) + (given_lap ? 1 : 0) + (lap_ae ? 1 : 0);
    StageTimer t(c, PF_STAGE_METRICS,
                 batch * ((double)gw * gh * 4.0 + (double)w * h * ((given16 ? 2.0 : 4.0) + 8.0 * planes)),
                 2);
    launch_edge(c->stream, j, c->metrics_ws.p, out);
    HIPCHK(c, hipGetLastError());
    return PF_OK;
}

int pf_error_compare(pf_ctx* c, const float* gt, int gw, int gh, int gc, const float* given, int w,
                     int h, int given_c, int batch, float zr0, float zr1, int disp_depth,
                     int align_way, int cap_depth, pf_compare* out, float* depth, uint8_t* shifted)
{
    int rc;
    if ((rc = check_device(c))) return rc;
    if (!gt || !given || !out) return fail(c, PF_EINVAL, "pf_error_compare: need gt, given and out");
    if (gw < 1 || gh < 1 || gc < 1 || w < 1 || h < 1 || given_c < 1)
        return fail(c, PF_EINVAL, "pf_error_compare: bad shape gt %dx%dx%d given %dx%dx%d", gw, gh,
                    gc, w, h, given_c);
    if (batch <= 0 || batch > 65535) return fail(c, PF_EINVAL, "batch %d out of range", batch);
    if (align_way < 0 || align_way > 2) return fail(c, PF_EINVAL, "align_way %d", align_way);
    // a block indexes up to 1024 units past the last pixel in an int
    const long long lim = (1ll << 31) - 4096;
    if ((long long)w * h >= lim || (long long)gw * gh * gc >= lim || (long long)w * h * given_c >= lim)
        return fail(c, PF_EINVAL, "pf_error_compare: map too large");
    const int n = w * h, ng = gw * gh;
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t o_fit = 0, o_m = o_fit + up(sizeof(pf_metrics) * batch),
                 o_cells = o_m + up(sizeof(pf_metrics) * batch),
                 o_gtd = o_cells + up(sizeof(uint32_t) * CMP_CELLS * batch),
                 o_depth = o_gtd + (disp_depth ? up(sizeof(float) * (size_t)ng * batch) : 0),
                 total = o_depth + (disp_depth && !depth ? up(sizeof(float) * (size_t)n * batch) : 0);
    if ((rc = ensure(c, c->cmp_ws, total))) return rc;
    char* ws = (char*)c->cmp_ws.p;
    pf_metrics* fit = (pf_metrics*)(ws + o_fit);
    pf_metrics* m = (pf_metrics*)(ws + o_m);
    uint32_t* cells = (uint32_t*)(ws + o_cells);
    if (!disp_depth) {
        // Depth.cpp:2606-2630: ErrorEmap, then the given map itself as 8 bits
        if ((rc = pf_error_metrics(c, gt, gw, gh, gc, given, nullptr, w, h, given_c, batch, zr0, zr1,
                                   align_way, cap_depth, m)))
            return rc;
        StageTimer t(c, PF_STAGE_METRICS,
                     (double)batch * n * (4.0 + (shifted ? 1.0 : 0.0) + (depth ? 4.0 : 0.0)), 2);
        if (shifted || depth) launch_cmp_quant(c->stream, given, given_c, n, batch, nullptr, shifted, depth);
        launch_cmp_final(c->stream, m, nullptr, nullptr, batch, out);
        HIPCHK(c, hipGetLastError());
        return PF_OK;
    }
    float* gt_disp = (float*)(ws + o_gtd);
    float* dplane = depth ? depth : (float*)(ws + o_depth);
    {   // Depth.cpp:2481-2487: the gt's disparity, one channel
        StageTimer t(c, PF_STAGE_METRICS, (double)batch * ng * 8.0, 2);
        launch_cmp_conv(c->stream, gt, gc, gt_disp, 1, ng, gc, batch);
        launch_cmp_init(c->stream, cells, batch);
        HIPCHK(c, hipGetLastError());
    }
    // Depth.cpp:2492: the least-squares fit of the given disparity to the gt's, no cap
    if ((rc = pf_error_metrics(c, gt_disp, gw, gh, 1, given, nullptr, w, h, given_c, batch, zr0, zr1,
                               2, 0, fit)))
        return rc;
    {   // Depth.cpp:2495-2527: affine, to depth, clip; and the min / max of :2537-2551
        StageTimer t(c, PF_STAGE_METRICS, (double)batch * n * (4.0 * given_c + 4.0), 1);
        launch_cmp_fused(c->stream, given, given_c, n, batch, fit, dplane, cells);
        HIPCHK(c, hipGetLastError());
    }
    // Depth.cpp:2530: the metrics proper, depth against depth
    if ((rc = pf_error_metrics(c, gt, gw, gh, gc, dplane, nullptr, w, h, 1, batch, zr0, zr1,
                               align_way, cap_depth, m)))
        return rc;
    StageTimer t(c, PF_STAGE_METRICS, shifted ? (double)batch * n * 5.0 : 0.0, shifted ? 2 : 1);
    if (shifted) launch_cmp_quant(c->stream, dplane, 1, n, batch, cells, shifted, nullptr);
    launch_cmp_final(c->stream, m, fit, cells, batch, out);
    HIPCHK(c, hipGetLastError());
    return PF_OK;
}

int pf_disp_depth_convert(pf_ctx* c, float* data, long long npix, int channels)
{
    int rc;
    if ((rc = check_device(c))) return rc;
    if (!data || npix < 0 || channels < 1)
        return fail(c, PF_EINVAL, "pf_disp_depth_convert: bad arguments");
    const long long chunk = 1ll << 30;  // pixels per launch (a multiple of 4: the alignment holds)
    for (long long p0 = 0; p0 < npix; p0 += chunk) {
        float* p = data + p0 * channels;
        launch_cmp_conv(c->stream, p, channels, p, channels, (int)std::min(chunk, npix - p0),
                        channels, 1);
    }
    HIPCHK(c, hipGetLastError());
    return PF_OK;
}

int pf_depth_transform(pf_ctx* c, float* data, long long npix, int channels, const float* abcd)
{
    int rc;
    if ((rc = check_device(c))) return rc;
    if (!data || !abcd || npix < 0 || channels < 1)
        return fail(c, PF_EINVAL, "pf_depth_transform: bad arguments");
    if (npix == 0) return PF_OK;
    launch_d2d_map(c->stream, data, npix, channels, abcd);
    HIPCHK(c, hipGetLastError());
    return PF_OK;
}

}  // extern "C"
