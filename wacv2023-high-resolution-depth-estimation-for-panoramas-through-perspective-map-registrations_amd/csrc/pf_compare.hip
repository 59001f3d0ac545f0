// The per-pixel steps of DepthNamespace::ErrorCompare (Depth.cpp:2460-2634) around its two
// ErrorEmap calls (pf_metrics.hip), and EquirectangularMap::DispDepthConversion (:587-610):
//   k_cmp_conv   channel 0 of a map to its reciprocal where (double)|v| >= 1e-5, `times` times
//                over (the reference loops over the channels but converts channel 0 each time);
//   k_cmp_fused  one pass over the given map: v = given * s + o with {s, o} read from the
//                pf_metrics that the fit call wrote on the device, conv, clip to [0, 10], the depth
//                plane, and min / max / count of the non-black values ((double)|v| >= 1e-4);
//   k_cmp_quant  (v - vmin) / (vmax - vmin) of the non-black values with vmin / vmax read from
//                the device, then (unsigned char)(max(v, 0) * 255.0f); quantise only in depth mode.
// All fp32, one rounding per operation (-ffp-contract=off, IEEE divide).  Rules where the
// reference is undefined: a product above 255 saturates to 255, NaN becomes 0 in the u8 plane;
// every comparison follows IEEE, so a NaN is not black, does not move vmin / vmax and stays NaN in
// the depth plane.
//
// After the clip every non-black, non-NaN value lies in [1e-4, 10], so its bit pattern orders as
// an unsigned integer: the min / max are a wave reduction, a block reduction through LDS and one
// unsigned atomic min / max / add per block into the panorama's cells -- exact and independent of
// the order.  k_cmp_init resets the cells on the stream before every call.
//
// A panorama is a flat run of n pixels at element offset b * n.  With one channel and 16-byte
// aligned bases the kernels move 16 bytes per lane: the (4 - b * n % 4) % 4 pixels ahead of the
// first aligned one and the up to 3 behind the last vector are scalar (block 0); any other layout
// (interleaved channels, odd bases) takes the scalar form of the same kernels.
#include "pf_internal.hpp"

#include <cfloat>

namespace pf {

namespace {

constexpr int CB = 256;  // threads per block
constexpr int CV = 4;    // units (16-byte vectors, or pixels in the scalar form) per thread

// (double)fabsf(v) < 1e-5 and < 1e-4 decided in fp32: each bound lies strictly between two
// neighbouring floats, so the test is |v| <= the lower one (false for NaN either way).
constexpr float CONV_KEEP = 0x1.4f8b58p-17f, CONV_FROM = 0x1.4f8b5ap-17f;
static_assert((double)CONV_KEEP < 1e-5 && (double)CONV_FROM >= 1e-5, "neighbours of 1e-5");
static_assert(__builtin_bit_cast(uint32_t, CONV_FROM) == __builtin_bit_cast(uint32_t, CONV_KEEP) + 1,
              "adjacent floats");
constexpr float BLACK_TO = 0x1.a36e2ep-14f, BLACK_FROM = 0x1.a36e30p-14f;
static_assert((double)BLACK_TO < 1e-4 && (double)BLACK_FROM >= 1e-4, "neighbours of 1e-4");
static_assert(__builtin_bit_cast(uint32_t, BLACK_FROM) == __builtin_bit_cast(uint32_t, BLACK_TO) + 1,
              "adjacent floats");
constexpr uint32_t FLT_MAX_BITS = 0x7f7fffffu;

__device__ __forceinline__ float conv_n(float v, int times)
{  // Depth.cpp:595-606, once per channel
    for (int k = 0; k < times; ++k)
        if (!(fabsf(v) <= CONV_KEEP)) v = 1.0f / v;
    return v;
}

__device__ __forceinline__ bool is_black(float v) { return fabsf(v) <= BLACK_TO; }

__device__ __forceinline__ uint32_t quant8(float v)
{  // Depth.cpp:2588-2593
    if (v < 0) v = 0;
    const float p = v * 255.0f;
    if (p != p) return 0u;
    return p >= 255.0f ? 255u : (uint32_t)p;
}

// The split of a panorama's n pixels at element offset `first` (b * n) of a 16-byte aligned base.
struct Span {
    int head, nvec, rest;  // scalar pixels ahead, 16-byte vectors, scalar pixels behind
};
__device__ __forceinline__ Span span_of(long long first, int n)
{
    Span s;
    s.head = (int)((4 - (first & 3)) & 3);
    if (s.head > n) s.head = n;
    s.nvec = (n - s.head) >> 2;
    s.rest = n - s.head - 4 * s.nvec;
    return s;
}
// Pixel index of the tid-th scalar pixel of a span (tid < head + rest).
__device__ __forceinline__ int scalar_px(const Span& s, int tid)
{
    return tid < s.head ? tid : s.head + 4 * s.nvec + (tid - s.head);
}

template <bool VEC>
__global__ __launch_bounds__(CB) void k_cmp_conv(const float* in, int in_c, float* out, int out_c,
                                                 int n, int times)
{
    const long long first = (long long)blockIdx.y * n;
    const int tid = threadIdx.x;
    const int u0 = blockIdx.x * (CB * CV) + tid;
    if (VEC) {
        const Span s = span_of(first, n);
        const float* src = in + first + s.head;
        float* dst = out + first + s.head;
        float4 x[CV];
#pragma unroll
        for (int k = 0; k < CV; ++k) {
            const int i = u0 + k * CB;
            if (i < s.nvec) x[k] = *reinterpret_cast<const float4*>(src + 4ll * i);
        }
#pragma unroll
        for (int k = 0; k < CV; ++k) {
            const int i = u0 + k * CB;
            if (i < s.nvec) {
                float4 r;
                r.x = conv_n(x[k].x, times);
                r.y = conv_n(x[k].y, times);
                r.z = conv_n(x[k].z, times);
                r.w = conv_n(x[k].w, times);
                *reinterpret_cast<float4*>(dst + 4ll * i) = r;
            }
        }
        if (blockIdx.x == 0 && tid < s.head + s.rest) {
            const int e = scalar_px(s, tid);
            out[first + e] = conv_n(in[first + e], times);
        }
    } else {
        float x[CV];
#pragma unroll
        for (int k = 0; k < CV; ++k) {
            const int i = u0 + k * CB;
            if (i < n) x[k] = in[(first + i) * in_c];
        }
#pragma unroll
        for (int k = 0; k < CV; ++k) {
            const int i = u0 + k * CB;
            if (i < n) out[(first + i) * out_c] = conv_n(x[k], times);
        }
    }
}

__global__ void k_cmp_init(uint32_t* cells, int batch)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    cells[b * CMP_CELLS + 0] = FLT_MAX_BITS;  // min: FLT_MAX when no pixel qualifies
    cells[b * CMP_CELLS + 1] = 0u;            // max: 0 = no pixel qualified (-FLT_MAX)
    cells[b * CMP_CELLS + 2] = 0u;            // count of non-black pixels
    cells[b * CMP_CELLS + 3] = 0u;
}

struct MinMax {
    uint32_t mn = 0xffffffffu, mx = 0u, cnt = 0u;
};
// Depth.cpp:2503, :2511, :2520-2523, then the min / max step of :2542-2549.
__device__ __forceinline__ float fused_px(float v, float s, float o, int times, MinMax& r)
{
    v = v * s;
    v = v + o;
    v = conv_n(v, times);
    if (v < 0) v = 0;
    if (v > 10.0f) v = 10.0f;
    if (!is_black(v)) {
        ++r.cnt;
        if (v == v) {
            const uint32_t bits = __float_as_uint(v);
            r.mn = min(r.mn, bits);
            r.mx = max(r.mx, bits);
        }
    }
    return v;
}

template <bool VEC>
__global__ __launch_bounds__(CB) void k_cmp_fused(const float* given, int given_c, int n,
                                                  const pf_metrics* fit, float* depth,
                                                  uint32_t* cells)
{
    const int b = blockIdx.y;
    const long long first = (long long)b * n;
    const int tid = threadIdx.x;
    const int u0 = blockIdx.x * (CB * CV) + tid;
    const float s = fit[b].ls_s, o = fit[b].ls_o;
    MinMax r;
    if (VEC) {
        const Span sp = span_of(first, n);
        const float* src = given + first + sp.head;
        float* dst = depth + first + sp.head;
        float4 x[CV];
#pragma unroll
        for (int k = 0; k < CV; ++k) {
            const int i = u0 + k * CB;
            if (i < sp.nvec) x[k] = *reinterpret_cast<const float4*>(src + 4ll * i);
        }
#pragma unroll
        for (int k = 0; k < CV; ++k) {
            const int i = u0 + k * CB;
            if (i < sp.nvec) {
                float4 q;
                q.x = fused_px(x[k].x, s, o, given_c, r);
                q.y = fused_px(x[k].y, s, o, given_c, r);
                q.z = fused_px(x[k].z, s, o, given_c, r);
                q.w = fused_px(x[k].w, s, o, given_c, r);
                *reinterpret_cast<float4*>(dst + 4ll * i) = q;
            }
        }
        if (blockIdx.x == 0 && tid < sp.head + sp.rest) {
            const int e = scalar_px(sp, tid);
            depth[first + e] = fused_px(given[first + e], s, o, given_c, r);
        }
    } else {
        float x[CV];
#pragma unroll
        for (int k = 0; k < CV; ++k) {
            const int i = u0 + k * CB;
            if (i < n) x[k] = given[(first + i) * given_c];
        }
#pragma unroll
        for (int k = 0; k < CV; ++k) {
            const int i = u0 + k * CB;
            if (i < n) depth[first + i] = fused_px(x[k], s, o, given_c, r);
        }
    }
    // wave, then block, then one atomic of each kind per block
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        r.mn = min(r.mn, (uint32_t)__shfl_xor((int)r.mn, d));
        r.mx = max(r.mx, (uint32_t)__shfl_xor((int)r.mx, d));
        r.cnt += (uint32_t)__shfl_xor((int)r.cnt, d);
    }
    __shared__ uint32_t part[CB / 64][3];
    if ((tid & 63) == 0) {
        part[tid >> 6][0] = r.mn;
        part[tid >> 6][1] = r.mx;
        part[tid >> 6][2] = r.cnt;
    }
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < CB / 64; ++k) {
            r.mn = min(r.mn, part[k][0]);
            r.mx = max(r.mx, part[k][1]);
            r.cnt += part[k][2];
        }
        uint32_t* c = cells + b * CMP_CELLS;
        if (r.mx != 0u) {
            atomicMin(c + 0, r.mn);
            atomicMax(c + 1, r.mx);
        }
        if (r.cnt != 0u) atomicAdd(c + 2, r.cnt);
    }
}

struct Norm {
    bool on;
    float vmin, den;
};
// Depth.cpp:2557-2563, then :2588-2593.
__device__ __forceinline__ uint32_t quant_px(float v, const Norm& nm)
{
    if (nm.on && !is_black(v)) v = (v - nm.vmin) / nm.den;
    return quant8(v);
}

template <bool VEC>
__global__ __launch_bounds__(CB) void k_cmp_quant(const float* src, int src_c, int n,
                                                  const uint32_t* cells, uint8_t* shifted,
                                                  float* copy)
{
    const int b = blockIdx.y;
    const long long first = (long long)b * n;
    const int tid = threadIdx.x;
    const int u0 = blockIdx.x * (CB * CV) + tid;
    Norm nm{cells != nullptr, 0.0f, 1.0f};
    if (cells) {
        const uint32_t mx = cells[b * CMP_CELLS + 1];
        nm.vmin = __uint_as_float(cells[b * CMP_CELLS + 0]);
        const float vmax = mx ? __uint_as_float(mx) : -FLT_MAX;
        nm.den = vmax - nm.vmin;
    }
    if (VEC) {  // src_c == 1, no copy
        const Span sp = span_of(first, n);
        const float* s4 = src + first + sp.head;
        uint8_t* d4 = shifted + first + sp.head;
        float4 x[CV];
#pragma unroll
        for (int k = 0; k < CV; ++k) {
            const int i = u0 + k * CB;
            if (i < sp.nvec) x[k] = *reinterpret_cast<const float4*>(s4 + 4ll * i);
        }
#pragma unroll
        for (int k = 0; k < CV; ++k) {
            const int i = u0 + k * CB;
            if (i < sp.nvec) {
                const uint32_t q = quant_px(x[k].x, nm) | quant_px(x[k].y, nm) << 8 |
                                   quant_px(x[k].z, nm) << 16 | quant_px(x[k].w, nm) << 24;
                *reinterpret_cast<uint32_t*>(d4 + 4ll * i) = q;
            }
        }
        if (blockIdx.x == 0 && tid < sp.head + sp.rest) {
            const int e = scalar_px(sp, tid);
            shifted[first + e] = (uint8_t)quant_px(src[first + e], nm);
        }
    } else {
        float x[CV];
#pragma unroll
        for (int k = 0; k < CV; ++k) {
            const int i = u0 + k * CB;
            if (i < n) x[k] = src[(first + i) * src_c];
        }
#pragma unroll
        for (int k = 0; k < CV; ++k) {
            const int i = u0 + k * CB;
            if (i < n) {
                if (copy) copy[first + i] = x[k];
                if (shifted) shifted[first + i] = (uint8_t)quant_px(x[k], nm);
            }
        }
    }
}

__global__ void k_cmp_final(const pf_metrics* m, const pf_metrics* fit, const uint32_t* cells,
                            int batch, pf_compare* out)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    pf_compare r;
    r.m = m[b];
    r.fit_s = fit ? fit[b].ls_s : 0.0f;
    r.fit_o = fit ? fit[b].ls_o : 0.0f;
    r.vmin = FLT_MAX;
    r.vmax = -FLT_MAX;
    r.n_nonblack = 0;
    if (cells) {
        const uint32_t mx = cells[b * CMP_CELLS + 1];
        r.vmin = __uint_as_float(cells[b * CMP_CELLS + 0]);
        if (mx) r.vmax = __uint_as_float(mx);
        r.n_nonblack = (int32_t)cells[b * CMP_CELLS + 2];
    }
    r.reserved[0] = r.reserved[1] = r.reserved[2] = 0;
    out[b] = r;
}

bool aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// Blocks along x for n pixels per panorama: CB * CV units each, at least one (the scalar
// pixels of the vector form belong to block 0).
unsigned blocks_for(int n, bool vec)
{
    const long long units = vec ? n / 4 : n;
    const long long g = (units + CB * CV - 1) / (CB * CV);
    return (unsigned)(g < 1 ? 1 : g);
}

}  // namespace

void launch_cmp_conv(hipStream_t s, const float* in, int in_c, float* out, int out_c, int n,
                     int times, int batch)
{
    const bool vec = in_c == 1 && out_c == 1 && aligned(in, 16) && aligned(out, 16);
    const dim3 grid(blocks_for(n, vec), (unsigned)batch);
    if (vec)
        hipLaunchKernelGGL(k_cmp_conv<true>, grid, dim3(CB), 0, s, in, in_c, out, out_c, n, times);
    else
        hipLaunchKernelGGL(k_cmp_conv<false>, grid, dim3(CB), 0, s, in, in_c, out, out_c, n, times);
}

void launch_cmp_init(hipStream_t s, uint32_t* cells, int batch)
{
    hipLaunchKernelGGL(k_cmp_init, dim3((batch + 255) / 256), dim3(256), 0, s, cells, batch);
}

void launch_cmp_fused(hipStream_t s, const float* given, int given_c, int n, int batch,
                      const pf_metrics* fit, float* depth, uint32_t* cells)
{
    const bool vec = given_c == 1 && aligned(given, 16) && aligned(depth, 16);
    const dim3 grid(blocks_for(n, vec), (unsigned)batch);
    if (vec)
        hipLaunchKernelGGL(k_cmp_fused<true>, grid, dim3(CB), 0, s, given, given_c, n, fit, depth,
                           cells);
    else
        hipLaunchKernelGGL(k_cmp_fused<false>, grid, dim3(CB), 0, s, given, given_c, n, fit, depth,
                           cells);
}

void launch_cmp_quant(hipStream_t s, const float* src, int src_c, int n, int batch,
                      const uint32_t* cells, uint8_t* shifted, float* copy)
{
    const bool vec = src_c == 1 && !copy && shifted && aligned(src, 16) && aligned(shifted, 4);
    const dim3 grid(blocks_for(n, vec), (unsigned)batch);
    if (vec)
        hipLaunchKernelGGL(k_cmp_quant<true>, grid, dim3(CB), 0, s, src, src_c, n, cells, shifted,
                           copy);
    else
        hipLaunchKernelGGL(k_cmp_quant<false>, grid, dim3(CB), 0, s, src, src_c, n, cells, shifted,
                           copy);
}

void launch_cmp_final(hipStream_t s, const pf_metrics* m, const pf_metrics* fit,
                      const uint32_t* cells, int batch, pf_compare* out)
{
    hipLaunchKernelGGL(k_cmp_final, dim3((batch + 255) / 256), dim3(256), 0, s, m, fit, cells,
                       batch, out);
}

}  // namespace pf
