// pf_stitch.hip -- two diagnostics of MergeDepthMaps / SolveDepthAll that the reference keeps
// behind `if (false)`, bit-exact on gfx950.
//
// The direct stitch (Depth.cpp:817-865): every output pixel takes the registered value of the
// FIRST tile whose range box contains it (both box ends inclusive, no zenith band, no fusion).
//  * k_stitch_map (layout-only): per pixel the first covering tile and its Value() index -- the
//    projection of the fusion grid (SphericalTo2D + Value's truncation from the same host sincos
//    tables as k_smooth_map), an index that leaves the tile clamped as k_smooth_map clamps it.
//  * k_stitch: per panorama the gather, the optional Depth2DepthTransform on the fly and the u16
//    quantisation.  A lane owns two adjacent pixels and stores them as one dword; the pairs are
//    cut relative to the plane's own address, so a plane that starts on an odd u16 offset keeps
//    aligned dword stores and only its first / last pixel is stored alone.
//
// The Laplacian self-check (Depth.cpp:1738-1758): the squared distance between a solved plane's
// 5-point Laplacian and the targets the sweeps pulled toward, summed in the reference's row-major
// order into a float (err += pow(d, 2): an exact double square per step, sq_step of
// pf_metrics.hip).  k_lap_residual: one wave per panorama; the lanes form 64 consecutive terms at
// a time (the next 64 are loaded while the current ones are added) and every lane runs the same
// chain over them, so the order is the reference's.  A diagnostic, not the step: ~40 cycles per
// pixel on the one wave.
#include "pf_internal.hpp"

namespace pf {

__global__ void __launch_bounds__(256) k_stitch_map(const TileGeom* __restrict__ geom,
                                                    const SmoothBox* __restrict__ box, int ntiles,
                                                    const GridCol* __restrict__ cols,
                                                    const GridRow* __restrict__ rows, int w, int h,
                                                    int2* __restrict__ src)
{
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= w * h) return;
    const int Y = i / w, X = i - Y * w;
    int first = -1;
    for (int p = 0; p < ntiles; p++) {  // ascending order, the first hit wins (:829-853)
        const SmoothBox b = box[p];
        if (X >= min(b.x0, b.x1) && X <= max(b.x0, b.x1) && Y >= b.y0 && Y <= b.y1) {
            first = p;
            break;
        }
    }
    int2 s = make_int2(-1, 0);
    if (first >= 0) {
        const TileGeom g = geom[first];
        const GridCol c = cols[X + 1];
        const GridRow r = rows[Y + 1];
        float x, y;
        sph_to_2d(g, r.sz, r.cz, c.ca, c.sa, x, y);
        long long idx = tile_index(g, x, y);
        const long long lim = (long long)g.w * g.h * g.c;
        if (idx < 0) idx = 0;  // out-of-tile tap: the reference reads out of bounds; clamp
        if (idx >= lim) idx = lim - g.c;
        s = make_int2(first, (int)idx);
    }
    src[i] = s;
}

__device__ __forceinline__ uint32_t stitch_px(const TileGeom* __restrict__ geom, int ntiles,
                                              int2 s, const float* __restrict__ tiles,
                                              const float* __restrict__ coeffs)
{
    if (s.x < 0) return 0u;  // memset(data, 0) (:814)
    float v = tiles[geom[s.x].off + s.y];
    if (coeffs) {
        const float4 k = *reinterpret_cast<const float4*>(coeffs + (long long)s.x * 4);
        v = cubic_map(v, k.x, k.y, k.z, k.w);
    }
    if (v < 0) v = 0;  // the library's quantiser (k_quantize)
    if (v > 1) v = 1;
    return (uint32_t)(uint16_t)(v * 65535.0f);
}

__global__ void __launch_bounds__(256) k_stitch(const TileGeom* __restrict__ geom, int ntiles,
                                                const int2* __restrict__ src, int npx,
                                                const float* __restrict__ tiles,
                                                long long tstride,
                                                const float* __restrict__ coeffs,
                                                uint16_t* __restrict__ out)
{
    const int b = blockIdx.y;
    uint16_t* const o = out + (long long)b * npx;
    // lane j owns pixels 2j - odd and 2j - odd + 1: that pair is dword-aligned in memory
    const int odd = (int)(((uintptr_t)o >> 1) & 1u);
    const int j = (int)blockIdx.x * 256 + (int)threadIdx.x;
    const int i0 = 2 * j - odd, i1 = i0 + 1;
    if (i0 >= npx) return;
    const float* const t = tiles + (long long)b * tstride;
    const float* const k = coeffs ? coeffs + (long long)b * ntiles * 4 : nullptr;
    const bool has0 = i0 >= 0, has1 = i1 < npx;
    const uint32_t q0 = has0 ? stitch_px(geom, ntiles, src[i0], t, k) : 0u;
    const uint32_t q1 = has1 ? stitch_px(geom, ntiles, src[i1], t, k) : 0u;
    if (has0 && has1) *reinterpret_cast<uint32_t*>(o + i0) = q0 | (q1 << 16);
    else if (has0) o[i0] = (uint16_t)q0;
    else if (has1) o[i1] = (uint16_t)q1;
}

// The stitch under the validity rule (pf_set_tile_validity): which tile a pixel takes depends on
// the data, so the cached first-tile map does not apply.  A pixel walks the tiles in ascending
// order and takes the first whose box holds it and whose sampled value is valid (its raw value
// passes the rule and, with coefficients, its transformed value is finite); 0 if there is none.
// The box test, the projection and the clamp are k_stitch_map's, the quantiser k_stitch's.
__global__ void __launch_bounds__(256) k_stitch_valid(const TileGeom* __restrict__ geom,
                                                      const SmoothBox* __restrict__ box,
                                                      int ntiles,
                                                      const GridCol* __restrict__ cols,
                                                      const GridRow* __restrict__ rows, int w,
                                                      int npx, const float* __restrict__ tiles,
                                                      long long tstride,
                                                      const float* __restrict__ coeffs, float vlo,
                                                      float vhi, uint16_t* __restrict__ out)
{
    const int b = blockIdx.y;
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= npx) return;
    const int Y = i / w, X = i - Y * w;
    const float* const t = tiles + (long long)b * tstride;
    const GridCol c = cols[X + 1];
    const GridRow r = rows[Y + 1];
    uint16_t q = 0;
    for (int p = 0; p < ntiles; p++) {
        const SmoothBox bx = box[p];
        if (!(X >= min(bx.x0, bx.x1) && X <= max(bx.x0, bx.x1) && Y >= bx.y0 && Y <= bx.y1))
            continue;
        const TileGeom& g = geom[p];
        float x, y;
        sph_to_2d(g, r.sz, r.cz, c.ca, c.sa, x, y);
        long long idx = tile_index(g, x, y);
        const long long lim = (long long)g.w * g.h * g.c;
        if (idx < 0) idx = 0;
        if (idx >= lim) idx = lim - g.c;
        const float raw = t[g.off + idx];
        float v = raw;
        if (coeffs) {
            const float4 k =
                *reinterpret_cast<const float4*>(coeffs + ((long long)b * ntiles + p) * 4);
            v = cubic_map(v, k.x, k.y, k.z, k.w);
        }
        if (!(tile_ok(raw, vlo, vhi) && isfinite(v))) continue;
        if (v < 0) v = 0;
        if (v > 1) v = 1;
        q = (uint16_t)(v * 65535.0f);
        break;
    }
    out[(long long)b * npx + i] = q;
}

__device__ __forceinline__ float lap_sq_step(float acc, float v)
{  // err += pow(d, 2) (Depth.cpp:1754): sq_step of pf_metrics.hip
    const double t = (double)v;
    return (float)((double)acc + t * t);
}

// term k of the chain: pixel (1 + k % (w-2), h0 + 1 + k / (w-2)); 0 past the end (a zero term
// leaves the chain's value as it is)
__device__ __forceinline__ float lap_term(const float* __restrict__ B,
                                          const uint32_t* __restrict__ Ln, int w, int iw, int h0,
                                          int k, int n)
{
    if (k >= n) return 0.0f;
    const int yy = k / iw;
    const int o = (h0 + 1 + yy) * w + 1 + (k - yy * iw);
    const float val = B[o];
    const float v0 = B[o - 1], v1 = B[o + 1], v2 = B[o - w], v3 = B[o + w];
    const float cur = val - (((v0 + v1) + v2) + v3) / 4.0f;
    const uint32_t lb = Ln[o];
    // an un-windowed pixel's target is LaplacianWindow's default 0 (Depth.h:268-271)
    const float L = lb == PF_NAN_MARKER ? 0.0f : __uint_as_float(lb);
    return cur - L;
}

__global__ void __launch_bounds__(64) k_lap_residual(const float* __restrict__ buf,
                                                     const float* __restrict__ lnorm, int w,
                                                     long long plane, int h0, int h1,
                                                     float* __restrict__ err)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    const float* const B = buf + (long long)b * plane;
    const uint32_t* const Ln = reinterpret_cast<const uint32_t*>(lnorm) + (long long)b * plane;
    const int iw = w - 2, n = (h1 - h0 - 1) * iw;
    float acc = 0.0f;
    float d = lap_term(B, Ln, w, iw, h0, lane, n);
    for (int k0 = 0; k0 < n; k0 += 64) {
        const float dn = lap_term(B, Ln, w, iw, h0, k0 + 64 + lane, n);
        const int db = __float_as_int(d);
#pragma unroll
        for (int j = 0; j < 64; j++)
            acc = lap_sq_step(acc, __int_as_float(__builtin_amdgcn_readlane(db, j)));
        d = dn;
    }
    if (lane == 0) err[b] = acc;
}

void launch_stitch_map(hipStream_t s, const TileGeom* geom, const SmoothBox* box, int ntiles,
                       const GridCol* cols, const GridRow* rows, int w, int h, int2* src)
{
    const int n = w * h;
    hipLaunchKernelGGL(k_stitch_map, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, geom,
                       box, ntiles, cols, rows, w, h, src);
}

void launch_stitch(hipStream_t s, const TileGeom* geom, int ntiles, const int2* src,
                   const float* tiles, long long tstride, const float* coeffs, int w, int h,
                   uint16_t* out, int batch)
{
    const int n = w * h;
    const int lanes = n / 2 + 1;  // pairs, plus the pixel an odd plane offset leaves alone
    hipLaunchKernelGGL(k_stitch, dim3((unsigned)((lanes + 255) / 256), batch), dim3(256), 0, s,
                       geom, ntiles, src, n, tiles, tstride, coeffs, out);
}

void launch_stitch_valid(hipStream_t s, const TileGeom* geom, const SmoothBox* box, int ntiles,
                         const GridCol* cols, const GridRow* rows, const float* tiles,
                         long long tstride, const float* coeffs, int w, int h, TileValid tv,
                         uint16_t* out, int batch)
{
    const int n = w * h;
    hipLaunchKernelGGL(k_stitch_valid, dim3((unsigned)((n + 255) / 256), batch), dim3(256), 0, s,
                       geom, box, ntiles, cols, rows, w, n, tiles, tstride, coeffs, tv.lo, tv.hi,
                       out);
}

void launch_lap_residual(hipStream_t s, const float* buf, const float* lnorm, int w, int h,
                         int h0, int h1, int batch, float* err)
{
    hipLaunchKernelGGL(k_lap_residual, dim3(batch), dim3(64), 0, s, buf, lnorm, w,
                       (long long)w * h, h0, h1, err);
}

}  // namespace pf
