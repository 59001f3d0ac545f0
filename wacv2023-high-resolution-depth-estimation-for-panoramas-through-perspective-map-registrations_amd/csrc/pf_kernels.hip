// pf_kernels.hip -- gfx950 kernels of the panorama-depth fusion path.
//
// Every kernel is HBM/L2-bandwidth or VALU bound; there is no dense contraction, so no MFMA.
// Layout: batch-major planes, row-major pixels; one workgroup-grid dimension walks pixels
// (coalesced 64-lane rows), grid.y walks the batch (or the tile for per-tile work).
#include "pf_internal.hpp"

namespace pf {

static constexpr int kBlock = 256;

__device__ __forceinline__ float bits_f(uint32_t u) { return __uint_as_float(u); }
__device__ __forceinline__ uint32_t f_bits(float f) { return __float_as_uint(f); }

// ---------------------------------------------------------------------------------------------
// Level-0 seed (Depth.cpp:1442-1465): rows [h0,h1] take ValueAtCoord of the pixel's spherical
// coordinate, other rows 0.
__global__ void __launch_bounds__(kBlock) k_seed0(const float* __restrict__ emap, int ew, int eh,
                                                  int ec, long long estride,
                                                  const GridCol* __restrict__ cols,
                                                  const GridRow* __restrict__ rows,
                                                  LevelDims L, float* __restrict__ buf,
                                                  long long bstride)
{
    long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    long long n = (long long)L.w * L.h;
    if (i >= n) return;
    int b = blockIdx.y;
    int y = (int)(i / L.w), x = (int)(i - (long long)y * L.w);
    float v = 0.0f;
    if (y >= L.h0 && y <= L.h1) {
        long long e = emap_index(cols[x + 1].az, rows[y + 1].zen, ew, eh, ec);
        v = emap[b * estride + e];
    }
    buf[b * bstride + i] = v;
}

// Nearest 2x upsample of the previous level (Depth.cpp:1467-1485).
__global__ void __launch_bounds__(kBlock) k_upsample(const float* __restrict__ prev,
                                                     long long pstride, LevelDims L,
                                                     float* __restrict__ buf, long long bstride)
{
    long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    long long n = (long long)L.w * L.h;
    if (i >= n) return;
    int b = blockIdx.y;
    int y = (int)(i / L.w), x = (int)(i - (long long)y * L.w);
    int wp = L.w / 2;
    buf[b * bstride + i] = prev[b * pstride + (long long)(y / 2) * wp + x / 2];
}

// ---------------------------------------------------------------------------------------------
// Laplacian target of tile p at pixel (X, Y): the 5-point mask in std::map key order
// (X-1,Y), (X,Y-1), (X,Y), (X,Y+1), (X+1,Y) with weights -1/4,-1/4,1,-1/4,-1/4, each tap
// projected through SphericalTo2D and read with Value() (Depth.cpp:1570-1606).  A tap whose
// linear index leaves the tile is clamped (the reference reads out of bounds there).
__device__ __forceinline__ float tap_value(const TileGeom& g, const float* __restrict__ tile,
                                           const GridCol& c, const GridRow& r, bool xform,
                                           float4 abcd)
{
    float x, y;
    sph_to_2d(g, r.sz, r.cz, c.ca, c.sa, x, y);
    long long idx = tile_index(g, x, y);
    long long lim = (long long)g.w * g.h * g.c;
    if (idx < 0) idx = 0;
    if (idx >= lim) idx = lim - g.c;
    float v = tile[idx];
    if (xform) v = cubic_map(v, abcd.x, abcd.y, abcd.z, abcd.w);
    return v;
}

__device__ __forceinline__ float target_one(const TileGeom& g, const float* __restrict__ tile,
                                            const GridCol* __restrict__ cols,
                                            const GridRow* __restrict__ rows, int X, int Y,
                                            bool xform, float4 abcd)
{
    float Lp = 0;
    Lp += tap_value(g, tile, cols[X], rows[Y + 1], xform, abcd) * -0.25f;      // (X-1, Y)
    Lp += tap_value(g, tile, cols[X + 1], rows[Y], xform, abcd) * -0.25f;      // (X, Y-1)
    Lp += tap_value(g, tile, cols[X + 1], rows[Y + 1], xform, abcd) * 1.0f;    // (X, Y)
    Lp += tap_value(g, tile, cols[X + 1], rows[Y + 2], xform, abcd) * -0.25f;  // (X, Y+1)
    Lp += tap_value(g, tile, cols[X + 2], rows[Y + 1], xform, abcd) * -0.25f;  // (X+1, Y)
    return Lp;
}

// X iterates x0, x0+xs, ... and stops before x1 (Depth.cpp:1565-1623).
__device__ __forceinline__ bool in_box(const TileBox& bx, int X, int Y)
{
    if (Y < bx.y0 || Y > bx.y1) return false;
    return bx.xs > 0 ? (X >= bx.x0 && X < bx.x1) : (X <= bx.x0 && X > bx.x1);
}

__global__ void __launch_bounds__(kBlock) k_normalize(const float* __restrict__ lsum,
                                                      const float* __restrict__ cnt,
                                                      LevelDims L, float* __restrict__ lnorm,
                                                      int r0, int r1)
{  // rows [r0, r1) of the band
    long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    long long nband = (long long)L.w * (r1 - r0);
    if (i >= nband) return;
    long long o = (long long)r0 * L.w + i;
    int Y = (int)(o / L.w);
    float n = cnt[o];
    float out;
    if (Y <= L.h0 || Y >= L.h1 || n == 0.0f) out = bits_f(PF_NAN_MARKER);
    else if (n == 1.0f) out = lsum[o];
    else out = lsum[o] * (1.0f / n);
    lnorm[o] = out;
}

// Coverage count of rows [r0, r1) of the band by ALL tiles (the n of pf_fuse_partial over every
// tile, from the boxes alone): layout-only, so a rank of the sharded fusion counts its own rows
// instead of receiving the other ranks' counts.
__global__ void __launch_bounds__(kBlock) k_coverage_rows(const TileBox* __restrict__ box,
                                                          int ntiles, LevelDims L,
                                                          float* __restrict__ cnt, int r0, int r1)
{
    long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    long long n = (long long)L.w * (r1 - r0);
    if (i >= n) return;
    const int Y = (int)(i / L.w) + r0, X = (int)(i - (long long)(Y - r0) * L.w);
    float c = 0.0f;
    if (Y > L.h0 && Y < L.h1)
        for (int p = 0; p < ntiles; p++) c += in_box(box[p], X, Y) ? 1.0f : 0.0f;
    cnt[(long long)Y * L.w + X] = c;
}

// dst[i] += src[i]: a received partial-target segment added into this rank's sums.  Exact for
// pixels covered by at most two tiles (one of the addends is zero, or the pair is the whole sum);
// the three-or-more pixels are re-added in tile order by pf_fuse_multicover_patch.
__global__ void __launch_bounds__(kBlock) k_rows_add(float* __restrict__ dst,
                                                     const float* __restrict__ src, long long n)
{
    const long long i = ((long long)blockIdx.x * kBlock + threadIdx.x) * 4;
    if (i + 3 < n) {
        float4 a = *reinterpret_cast<const float4*>(dst + i);
        const float4 b = *reinterpret_cast<const float4*>(src + i);
        a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
        *reinterpret_cast<float4*>(dst + i) = a;
    } else {
        for (long long j = i; j < n; j++) dst[j] += src[j];
    }
}

// Several segments in one launch (pf_rows_add_batch): blockIdx.y = segment.
__global__ void __launch_bounds__(kBlock) k_rows_add_batch(RowsAddBatch B)
{
    const int k = blockIdx.y;
    float* __restrict__ dst = B.dst[k];
    const float* __restrict__ src = B.src[k];
    const long long n = B.n[k];
    for (long long i = ((long long)blockIdx.x * kBlock + threadIdx.x) * 4; i < n;
         i += (long long)gridDim.x * kBlock * 4) {
        if (i + 3 < n && ((reinterpret_cast<uintptr_t>(dst + i) | reinterpret_cast<uintptr_t>(src + i)) & 15) == 0) {
            float4 a = *reinterpret_cast<const float4*>(dst + i);
            const float4 b = *reinterpret_cast<const float4*>(src + i);
            a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
            *reinterpret_cast<float4*>(dst + i) = a;
        } else {
            for (long long j = i; j < n && j < i + 4; j++) dst[j] += src[j];
        }
    }
}

// Parity probe: linear tile index of each tap of the first covering tile.
__global__ void __launch_bounds__(kBlock) k_probe_taps(const TileGeom* __restrict__ geom,
                                                       const TileBox* __restrict__ box,
                                                       int ntiles,
                                                       const GridCol* __restrict__ cols,
                                                       const GridRow* __restrict__ rows,
                                                       LevelDims L, int32_t* __restrict__ out)
{
    long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    long long n = (long long)L.w * L.h;
    if (i >= n) return;
    int Y = (int)(i / L.w), X = (int)(i - (long long)Y * L.w);
    int32_t r[5] = {-1, -1, -1, -1, -1};
    if (Y > L.h0 && Y < L.h1) {
        for (int p = 0; p < ntiles; p++) {
            if (!in_box(box[p], X, Y)) continue;
            const TileGeom& g = geom[p];
            const int dc[5] = {0, 1, 1, 1, 2}, dr[5] = {1, 0, 1, 2, 1};
            for (int k = 0; k < 5; k++) {
                float x, y;
                const GridCol& c = cols[X + dc[k]];
                const GridRow& rr = rows[Y + dr[k]];
                sph_to_2d(g, rr.sz, rr.cz, c.ca, c.sa, x, y);
                r[k] = (int32_t)tile_index(g, x, y);
            }
            break;
        }
    }
    for (int k = 0; k < 5; k++) out[i * 5 + k] = r[k];
}

// ---------------------------------------------------------------------------------------------
// One damped Jacobi sweep over the band rows (Depth.cpp:1680-1717).  Taps are read by linear
// index so the east tap of column w-1 is pixel (0, Y+1), exactly like buffer[yy*width+xx].
__global__ void __launch_bounds__(kBlock) k_jacobi(const float* __restrict__ src,
                                                   float* __restrict__ dst,
                                                   const float* __restrict__ lnorm,
                                                   long long stride, LevelDims L)
{
    long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    long long nband = (long long)L.w * (L.h1 - L.h0 + 1);
    if (i >= nband) return;
    long long base = (long long)blockIdx.y * stride;
    long long o = (long long)L.h0 * L.w + i;
    const float* s = src + base;
    float Lt = lnorm[base + o];
    float b = s[o];
    float cur = 0.0f, tgt = 0.0f;
    if (f_bits(Lt) != PF_NAN_MARKER) {
        tgt = Lt;
        cur += s[o - 1] * -0.25f;
        cur += s[o - L.w] * -0.25f;
        cur += b * 1.0f;
        cur += s[o + L.w] * -0.25f;
        cur += s[o + 1] * -0.25f;
    }
    const float reg = (float)1e-4;
    const float reg_ = 1 - reg;
    float target_val = b + (tgt - cur) * 0.5f;
    float v = target_val * reg_ + b * reg;
    if (v < 0) v = 0;
    else if (v > 1) v = 1;
    dst[base + o] = v;
}

__global__ void __launch_bounds__(kBlock) k_quantize(const float* __restrict__ buf,
                                                     long long bstride, int n,
                                                     uint16_t* __restrict__ out,
                                                     long long ostride)
{
    long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    int b = blockIdx.y;
    float v = buf[b * bstride + i];
    if (v < 0) v = 0;
    if (v > 1) v = 1;
    out[b * ostride + i] = (uint16_t)(v * 65535.0f);
}

// Pixels covered by three or more tiles (pf_fuse_multicover, sharded fusion): the contribution
// of tile p to pixel o for every listed (o, p) pair with p in [t0, t1), 0 for the others.
__global__ void __launch_bounds__(kBlock) k_multicover_contrib(
    const TileGeom* __restrict__ geom, const int2* __restrict__ pairs, int npairs, int t0, int t1,
    const GridCol* __restrict__ cols, const GridRow* __restrict__ rows,
    const float* __restrict__ tiles, const float* __restrict__ coeffs, LevelDims L,
    float* __restrict__ contrib)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= npairs) return;
    const int o = pairs[i].x, p = pairs[i].y;
    float v = 0.0f;
    if (p >= t0 && p < t1) {
        const int Y = o / L.w, X = o - Y * L.w;
        const TileGeom& g = geom[p];
        float4 abcd = make_float4(0, 0, 0, 0);
        const bool xf = coeffs != nullptr;
        if (xf) abcd = *reinterpret_cast<const float4*>(coeffs + (long long)p * 4);
        v = target_one(g, tiles + g.off, cols, rows, X, Y, xf, abcd);
    }
    contrib[i] = v;
}

// The window sums of those pixels in the reference's single-thread order (tiles ascending, from
// 0, one rounding per tile), overwriting the rank-summed values; pairs are sorted by pixel, then
// tile.  One thread: a handful of pixels per level.
__global__ void k_multicover_patch(const int2* __restrict__ pairs, int npairs,
                                   const float* __restrict__ contrib, float* __restrict__ lsum)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int i = 0;
    while (i < npairs) {
        const int o = pairs[i].x;
        float acc = 0.0f;
        for (; i < npairs && pairs[i].x == o; i++) acc += contrib[i];
        lsum[o] = acc;
    }
}

// E->P RGB warp with the GL camera (a18): the taps (corners, weights) come from the host table
// (rgb_taps_host, glibc double atan2 as the oracle); per channel the GL_LINEAR blend in fp32 and
// the round-to-nearest u8 store.
__global__ void __launch_bounds__(kBlock) k_warp_rgb(const RgbTap* __restrict__ taps,
                                                     const TileGeom* __restrict__ geom,
                                                     const long long* __restrict__ rgb_off,
                                                     const uint8_t* __restrict__ pano, int pw,
                                                     int ph, long long pstride,
                                                     uint8_t* __restrict__ tiles,
                                                     long long tstride, int batch)
{
    const int p = blockIdx.y;
    const int W = geom[p].w, H = geom[p].h;
    long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (long long)W * H) return;
    const RgbTap t = taps[geom[p].pix_off + i];
    const float ax = t.ax, ay = t.ay;
    const long long ix0 = t.x0y0 & 0xFFFFu, iy0 = t.x0y0 >> 16;
    const long long ix1 = t.x1y1 & 0xFFFFu, iy1 = t.x1y1 >> 16;
    long long a00 = (iy0 * pw + ix0) * 3, a01 = (iy0 * pw + ix1) * 3;
    long long a10 = (iy1 * pw + ix0) * 3, a11 = (iy1 * pw + ix1) * 3;
    for (int b = 0; b < batch; b++) {
        const uint8_t* pp = pano + b * pstride;
        uint8_t* out = tiles + b * tstride + rgb_off[p] + i * 3;
        for (int ch = 0; ch < 3; ch++) {
            float t00 = pp[a00 + ch], t01 = pp[a01 + ch], t10 = pp[a10 + ch], t11 = pp[a11 + ch];
            float top = t00 * (1.0f - ax) + t01 * ax;
            float bot = t10 * (1.0f - ax) + t11 * ax;
            float v = top * (1.0f - ay) + bot * ay;
            int q = (int)floorf(v + 0.5f);
            q = q < 0 ? 0 : (q > 255 ? 255 : q);
            out[ch] = (uint8_t)q;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Launchers.
static inline unsigned nblocks(long long n) { return (unsigned)((n + kBlock - 1) / kBlock); }

void launch_seed0(hipStream_t s, const float* emap, int ew, int eh, int ec, long long estride,
                  const GridCol* cols, const GridRow* rows, LevelDims L, float* buf,
                  long long bstride, int batch)
{
    dim3 grid(nblocks((long long)L.w * L.h), batch);
    hipLaunchKernelGGL(k_seed0, grid, dim3(kBlock), 0, s, emap, ew, eh, ec, estride, cols, rows,
                       L, buf, bstride);
}

void launch_upsample(hipStream_t s, const float* prev, long long pstride, LevelDims L,
                     float* buf, long long bstride, int batch)
{
    dim3 grid(nblocks((long long)L.w * L.h), batch);
    hipLaunchKernelGGL(k_upsample, grid, dim3(kBlock), 0, s, prev, pstride, L, buf, bstride);
}

void launch_coverage_rows(hipStream_t s, const TileBox* box, int ntiles, LevelDims L, float* cnt,
                          int r0, int r1)
{
    if (r1 <= r0) return;
    hipLaunchKernelGGL(k_coverage_rows, dim3(nblocks((long long)L.w * (r1 - r0))), dim3(kBlock),
                       0, s, box, ntiles, L, cnt, r0, r1);
}

void launch_rows_add(hipStream_t s, float* dst, const float* src, long long n)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_rows_add, dim3(nblocks((n + 3) / 4)), dim3(kBlock), 0, s, dst, src, n);
}

void launch_rows_add_batch(hipStream_t s, const RowsAddBatch& B, int count, long long nmax)
{
    if (count <= 0 || nmax <= 0) return;
    long long nb = (nmax + 4LL * kBlock - 1) / (4LL * kBlock);
    if (nb > 1024) nb = 1024;
    hipLaunchKernelGGL(k_rows_add_batch, dim3((unsigned)nb, (unsigned)count), dim3(kBlock), 0, s, B);
}

void launch_multicover(hipStream_t s, const TileGeom* geom, const int2* pairs, int npairs,
                       int t0, int t1, const GridCol* cols, const GridRow* rows,
                       const float* tiles, const float* coeffs, LevelDims L, float* contrib)
{
    if (npairs <= 0) return;
    hipLaunchKernelGGL(k_multicover_contrib, dim3(nblocks(npairs)), dim3(kBlock), 0, s, geom, pairs,
                       npairs, t0, t1, cols, rows, tiles, coeffs, L, contrib);
}

void launch_multicover_patch(hipStream_t s, const int2* pairs, int npairs, const float* contrib,
                             float* lsum)
{
    if (npairs <= 0) return;
    hipLaunchKernelGGL(k_multicover_patch, dim3(1), dim3(64), 0, s, pairs, npairs, contrib, lsum);
}

void launch_normalize(hipStream_t s, const float* lsum, const float* cnt, LevelDims L,
                      float* lnorm, int r0, int r1)
{
    if (r0 < 0) { r0 = L.h0; r1 = L.h1 + 1; }
    if (r1 <= r0) return;
    dim3 grid(nblocks((long long)L.w * (r1 - r0)));
    hipLaunchKernelGGL(k_normalize, grid, dim3(kBlock), 0, s, lsum, cnt, L, lnorm, r0, r1);
}

void launch_probe_taps(hipStream_t s, const TileGeom* geom, const TileBox* box, int ntiles,
                       const GridCol* cols, const GridRow* rows, LevelDims L, int32_t* out)
{
    dim3 grid(nblocks((long long)L.w * L.h));
    hipLaunchKernelGGL(k_probe_taps, grid, dim3(kBlock), 0, s, geom, box, ntiles, cols, rows, L,
                       out);
}

void launch_jacobi(hipStream_t s, float* buf_a, float* buf_b, const float* lnorm,
                   long long stride, LevelDims L, int iters, int batch, float** result)
{
    dim3 grid(nblocks((long long)L.w * (L.h1 - L.h0 + 1)), batch);
    float* src = buf_a;
    float* dst = buf_b;
    for (int it = 0; it < iters; it++) {
        hipLaunchKernelGGL(k_jacobi, grid, dim3(kBlock), 0, s, src, dst, lnorm, stride, L);
        float* t = src;
        src = dst;
        dst = t;
    }
    *result = src;
}

void launch_quantize(hipStream_t s, const float* buf, long long bstride, int n, uint16_t* out,
                     long long ostride, int batch)
{
    dim3 grid(nblocks(n), batch);
    hipLaunchKernelGGL(k_quantize, grid, dim3(kBlock), 0, s, buf, bstride, n, out, ostride);
}

void launch_warp_rgb(hipStream_t s, const RgbTap* taps, const TileGeom* geom, int ntiles,
                     long long npix_max, const long long* rgb_off, const uint8_t* pano, int pw,
                     int ph, long long pstride, uint8_t* tiles, long long tstride, int batch)
{
    dim3 grid(nblocks(npix_max), ntiles);
    hipLaunchKernelGGL(k_warp_rgb, grid, dim3(kBlock), 0, s, taps, geom, rgb_off, pano, pw, ph,
                       pstride, tiles, tstride, batch);
}

}  // namespace pf
