// pf_global_api.hip -- the entry points of the post-fusion calibration tools: pf_register_global,
// pf_result_transform (SolveDepthToDepth2 and its u16 transform), pf_median_scale,
// pf_copy_invalid.  None of them needs a tile layout.
#include "pf_ctx.hpp"

#include <cmath>

using namespace pf;

namespace {

// The band rows of SolveDepthToDepth2 (Depth.cpp:1166-1167: the expression of level_dims for the
// last level).  The reference reads rows h0..h1 of the u16 plane unchecked; here they must exist.
int global_band(pf_ctx* c, const char* who, int out_w, int out_h, float zr0, float zr1, int* h0,
                int* h1)
{
    if (out_w < 2 || out_h < 2) return fail(c, PF_EINVAL, "%s: bad size %dx%d", who, out_w, out_h);
    const double a = floor((double)((float)out_h * zr0) / PF_MYPI);
    const double b = ceil((double)((float)out_h * zr1) / PF_MYPI);
    if (!(a >= 0.0 && a <= b && b <= (double)(out_h - 1)))
        return fail(c, PF_EINVAL, "%s: zenith range (%g, %g) gives rows %g..%g outside 0..%d", who,
                    (double)zr0, (double)zr1, a, b, out_h - 1);
    if ((double)out_w * (b - a + 1.0) >= 1073741824.0)  // 32-bit sample indices with headroom
        return fail(c, PF_EINVAL, "%s: %dx%d has too many band samples", who, out_w, out_h);
    *h0 = (int)a;
    *h1 = (int)b;
    return PF_OK;
}

// ValueAtCoord's index of sample (X, Y) split into its column and row terms (emap_index is
// separable), with the fp64 arithmetic of emap_index and SolveDepthToDepth2's coordinates
// (Depth.cpp:1198): built once per (result size, baseline size).
int global_tables(pf_ctx* c, int out_w, int out_h, int ew, int eh, int ec)
{
    const int key[5] = {out_w, out_h, ew, eh, ec};
    if (memcmp(key, c->glob_key, sizeof(key)) == 0) return PF_OK;
    std::vector<int> ecol(out_w), erow(out_h);
    for (int X = 0; X < out_w; X++) {
        const float az = (float)((double)((float)X / (float)(out_w - 1) * 2) * PF_MYPI);
        const long long e = emap_index(az, 0.0f, ew, eh, ec);
        if (e < 0 || e >= (long long)ew * ec) return fail(c, PF_EINVAL, "baseline column of X=%d out of range", X);
        ecol[X] = (int)e;
    }
    for (int Y = 0; Y < out_h; Y++) {
        const float zen = (float)((double)((float)Y / (float)(out_h - 1)) * PF_MYPI);
        const long long e = emap_index(0.0f, zen, ew, eh, ec);
        if (e < 0 || e > (long long)(eh - 1) * ew * ec) return fail(c, PF_EINVAL, "baseline row of Y=%d out of range", Y);
        erow[Y] = (int)e;
    }
    c->glob_key[0] = 0;
    int rc;
    if ((rc = upload(c, c->glob_ecol, ecol))) return rc;
    if ((rc = upload(c, c->glob_erow, erow))) return rc;
    memcpy(c->glob_key, key, sizeof(key));
    return PF_OK;
}

int check_map(pf_ctx* c, const char* who, const void* p, int w, int h, int ch, int batch)
{
    if (!p || w < 1 || h < 1 || ch < 1)
        return fail(c, PF_EINVAL, "%s: bad map %p %dx%dx%d", who, p, w, h, ch);
    if ((long long)w * h >= (1LL << 30))  // 32-bit pixel indices with headroom
        return fail(c, PF_EINVAL, "%s: map %dx%d too large", who, w, h);
    if (batch <= 0 || batch > 32767) return fail(c, PF_EINVAL, "batch %d out of range", batch);
    return PF_OK;
}

}  // namespace

extern "C" {

int pf_register_global(pf_ctx* c, const float* emap, int ew, int eh, int ec, uint16_t* data,
                       int batch, int out_w, int out_h, float zr0, float zr1, int apply,
                       float* coeffs, double* coeffs64, double* summary)
{
    int rc, h0, h1;
    if ((rc = check_device(c))) return rc;
    if ((rc = check_no_loss(c, "pf_register_global"))) return rc;
    if (batch <= 0 || batch > 65535) return fail(c, PF_EINVAL, "batch %d out of range", batch);
    if ((rc = check_emap(c, emap, ew, eh, ec))) return rc;
    if (!data) return fail(c, PF_EINVAL, "pf_register_global: data is NULL");
    if ((rc = global_band(c, "pf_register_global", out_w, out_h, zr0, zr1, &h0, &h1))) return rc;
    if ((rc = global_tables(c, out_w, out_h, ew, eh, ec))) return rc;
    const int ns = out_w * (h1 - h0 + 1);
    const int nchunks = (ns + kGlobalChunk - 1) / kGlobalChunk;
    const size_t part_bytes =
        (sizeof(double) * register_sums_per_tile() * (size_t)nchunks * batch + 15) & ~(size_t)15;
    if ((rc = ensure(c, c->glob_ws, part_bytes + sizeof(float) * 4 * batch))) return rc;
    double* partials = (double*)c->glob_ws.p;
    float* cf = coeffs ? coeffs : (float*)((char*)c->glob_ws.p + part_bytes);
    const long long dstride = (long long)out_w * out_h;
    {
        StageTimer t(c, PF_STAGE_REGISTER,
                     batch * ((double)ns * (2.0 + 4.0) + (apply ? 4.0 * ns : 0.0)), apply ? 3 : 2);
        launch_global_sums(c->stream, data, dstride, emap, (long long)ew * eh * ec,
                           (const int*)c->glob_ecol.p, (const int*)c->glob_erow.p, out_w, h0, ns,
                           nchunks, partials, batch);
        launch_global_solve(c->stream, partials, nchunks, batch, cf, coeffs64, summary);
        if (apply)
            launch_result_transform(c->stream, data, dstride, (long long)h0 * out_w, ns, cf, batch);
    }
    HIPCHK(c, hipGetLastError());
    return PF_OK;
}

int pf_result_transform(pf_ctx* c, uint16_t* data, int batch, int out_w, int out_h, float zr0,
                        float zr1, const float* coeffs)
{
    int rc, h0, h1;
    if ((rc = check_device(c))) return rc;
    if (batch <= 0 || batch > 65535) return fail(c, PF_EINVAL, "batch %d out of range", batch);
    if (!data || !coeffs) return fail(c, PF_EINVAL, "pf_result_transform: data/coeffs is NULL");
    if ((rc = global_band(c, "pf_result_transform", out_w, out_h, zr0, zr1, &h0, &h1))) return rc;
    launch_result_transform(c->stream, data, (long long)out_w * out_h, (long long)h0 * out_w,
                            out_w * (h1 - h0 + 1), coeffs, batch);
    HIPCHK(c, hipGetLastError());
    return PF_OK;
}

int pf_median_scale(pf_ctx* c, float* map0, int w0, int h0, int c0, const float* map1, int w1,
                    int h1, int c1, int batch, float* medians, int* status)
{
    int rc;
    if ((rc = check_device(c))) return rc;
    if ((rc = check_map(c, "pf_median_scale", map0, w0, h0, c0, batch))) return rc;
    if ((rc = check_map(c, "pf_median_scale", map1, w1, h1, c1, batch))) return rc;
    if ((rc = ensure(c, c->med_ws, median_workspace_bytes(batch)))) return rc;
    launch_median_scale(c->stream, map0, w0, h0, c0, map1, w1, h1, c1, batch, c->med_ws.p, medians,
                        status);
    HIPCHK(c, hipGetLastError());
    return PF_OK;
}

int pf_copy_invalid(pf_ctx* c, float* dst, int w, int h, int ch, const float* ref, int rw, int rh,
                    int rc_, int batch)
{
    int rc;
    if ((rc = check_device(c))) return rc;
    if ((rc = check_map(c, "pf_copy_invalid", dst, w, h, ch, batch))) return rc;
    if ((rc = check_map(c, "pf_copy_invalid", ref, rw, rh, rc_, batch))) return rc;
    launch_copy_invalid(c->stream, dst, w, h, ch, ref, rw, rh, rc_, batch);
    HIPCHK(c, hipGetLastError());
    return PF_OK;
}

}  // extern "C"
