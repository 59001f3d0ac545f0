// pf_global.hip -- the post-fusion calibration tools: the global result-to-baseline cubic fit
// (SolveDepthToDepth2, Depth.cpp:1158-1259) with its u16 transform, MedianScaling
// (Depth.cpp:637-701) and EquirectangularMap::CopyInvalidPixels (Depth.cpp:703-725).
//
// All of it streams one or two maps once per pass: bandwidth bound, no contraction, no MFMA.
#include "pf_internal.hpp"

namespace pf {

static constexpr int kBlock = 256;

// ---------------------------------------------------------------------------------------------
// Global cubic fit: the 15 fp64 moment sums of k_register (pf_register.hip: same products, same
// order per sample) over the samples s = (Y - h0) * W + X of rows h0..h1.  The order is fixed
// and independent of the grid: chunks of kGlobalChunk consecutive samples, one 256-lane block per
// (panorama, chunk); lane l adds its samples l, l + 256, ... of the chunk in order from 0.0; the
// halving tree of k_register reduces the chunk; k_global_solve (pf_register.hip) adds the chunk
// partials in chunk order.  No atomics.
static constexpr int kGlobalSums = 15;

__device__ __forceinline__ double clamp_sample(double v)
{
    if (v < 1e-4) v = 1e-4;
    else if (v > (1 - 1e-4)) v = 1 - 1e-4;
    return v;
}

__global__ void __launch_bounds__(kBlock) k_global_sums(
    const uint16_t* __restrict__ data, long long dstride, const float* __restrict__ emap,
    long long estride, const int* __restrict__ ecol, const int* __restrict__ erow, int w, int h0,
    int ns, int nchunks, double* __restrict__ partials)
{
    __shared__ double part[kGlobalSums][kBlock];
    const int ch = blockIdx.x, b = blockIdx.y, l = threadIdx.x;
    // the band's samples are contiguous in the u16 plane: s = (Y - h0) * W + X
    const uint16_t* d = data + b * dstride + (long long)h0 * w;
    const float* em = emap + b * estride;
    const int s_begin = ch * kGlobalChunk;
    const int s_end = ns - s_begin < kGlobalChunk ? ns : s_begin + kGlobalChunk;
    double acc[kGlobalSums];
#pragma unroll
    for (int k = 0; k < kGlobalSums; k++) acc[k] = 0.0;
    // groups of kU samples: their loads are issued together, then added in sample order (the
    // same per-lane order as one sample per iteration).  (row, column) of the lane's sample: one
    // division for its first sample, then steps of 256 samples = (256 / w) rows and (256 % w)
    // columns with one carry.
    constexpr int kU = 8;
    const int step_r = kBlock / w, step_x = kBlock - step_r * w;
    int r = (s_begin + l) / w, X = (s_begin + l) - r * w;
    for (int s0 = s_begin + l; s0 < s_end; s0 += kU * kBlock) {
        float xv[kU], yv[kU];
        int eidx[kU];
#pragma unroll
        for (int u = 0; u < kU; u++) {  // the index tables first: the gathers depend on them
            const int s = s0 + u * kBlock;
            eidx[u] = s < s_end ? erow[h0 + r] + ecol[X] : 0;
            r += step_r;
            X += step_x;
            if (X >= w) {
                X -= w;
                r++;
            }
        }
#pragma unroll
        for (int u = 0; u < kU; u++) {
            const int s = s0 + u * kBlock;
            xv[u] = 0.0f;
            yv[u] = 0.0f;
            if (s >= s_end) continue;
            xv[u] = u16_unit(d[s]);  // (float)data / 65535.0f, Depth.cpp:1200
            yv[u] = em[eidx[u]];
        }
#pragma unroll
        for (int u = 0; u < kU; u++) {
            if (s0 + u * kBlock >= s_end) break;
            const double X = clamp_sample((double)xv[u]);
            const double Yv = clamp_sample((double)yv[u]);
            const double X2 = X * X, X3 = X * X * X;
            acc[0] = acc[0] + X3 * X3; acc[1] = acc[1] + X3 * X2; acc[2] = acc[2] + X3 * X;
            acc[3] = acc[3] + X3;      acc[4] = acc[4] + X2 * X2; acc[5] = acc[5] + X2 * X;
            acc[6] = acc[6] + X2;      acc[7] = acc[7] + X * X;   acc[8] = acc[8] + X;
            acc[9] = acc[9] + 1.0;
            acc[10] = acc[10] + X3 * Yv; acc[11] = acc[11] + X2 * Yv; acc[12] = acc[12] + X * Yv;
            acc[13] = acc[13] + Yv;
            acc[14] = acc[14] + Yv * Yv;
        }
    }
#pragma unroll
    for (int k = 0; k < kGlobalSums; k++) part[k][l] = acc[k];
    __syncthreads();
    for (int stride = kBlock / 2; stride >= 1; stride >>= 1) {
        if (l < stride)
            for (int k = 0; k < kGlobalSums; k++) part[k][l] = part[k][l] + part[k][l + stride];
        __syncthreads();
    }
    if (l < kGlobalSums) partials[((long long)b * nchunks + ch) * kGlobalSums + l] = part[l][0];
}

void launch_global_sums(hipStream_t s, const uint16_t* data, long long dstride, const float* emap,
                        long long estride, const int* ecol, const int* erow, int w, int h0,
                        int ns, int nchunks, double* partials, int batch)
{
    hipLaunchKernelGGL(k_global_sums, dim3((unsigned)nchunks, (unsigned)batch), dim3(kBlock), 0, s,
                       data, dstride, emap, estride, ecol, erow, w, h0, ns, nchunks, partials);
}

// The cubic on n consecutive u16 values of each panorama (the band rows), in place:
// v = (float)d / 65535.0f, Depth2DepthTransform's map (cubic_map: left-associated fp32, clamps),
// NaN -> 0, (u16)(Y * 65535.0f).
__device__ __forceinline__ uint32_t cubic_u16(uint32_t d, const float4 q)
{
    float y = cubic_map(u16_unit(d), q.x, q.y, q.z, q.w);
    if (!(y == y)) y = 0.0f;
    return (uint32_t)(uint16_t)(y * 65535.0f);
}

__global__ void __launch_bounds__(kBlock) k_result_transform(uint16_t* __restrict__ data,
                                                             long long dstride, long long first,
                                                             int n, const float* __restrict__ coeffs)
{
    const int b = blockIdx.y;
    const float* cf = coeffs + (long long)b * 4;
    const float4 q = make_float4(cf[0], cf[1], cf[2], cf[3]);
    uint16_t* d = data + b * dstride + first;
    // eight values (16 bytes) per lane where the band of this panorama is 16-byte aligned
    const bool vec = (reinterpret_cast<uintptr_t>(d) & 15) == 0;
    const int n8 = vec ? n / 8 : 0;
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < n8; i += gridDim.x * kBlock) {
        uint4 v = reinterpret_cast<uint4*>(d)[i];
        uint32_t* p = &v.x;
#pragma unroll
        for (int k = 0; k < 4; k++)
            p[k] = cubic_u16(p[k] & 0xFFFFu, q) | (cubic_u16(p[k] >> 16, q) << 16);
        reinterpret_cast<uint4*>(d)[i] = v;
    }
    for (int i = n8 * 8 + blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock)
        d[i] = (uint16_t)cubic_u16(d[i], q);
}

void launch_result_transform(hipStream_t s, uint16_t* data, long long dstride, long long first,
                             int n, const float* coeffs, int batch)
{
    if (n <= 0) return;
    unsigned gx = (unsigned)((n / 8 + kBlock - 1) / kBlock);
    if (gx > 1024) gx = 1024;
    if (gx == 0) gx = 1;
    hipLaunchKernelGGL(k_result_transform, dim3(gx, (unsigned)batch), dim3(kBlock), 0, s, data,
                       dstride, first, n, coeffs);
}

// ---------------------------------------------------------------------------------------------
// MedianScaling.  A pixel is valid when !(v < 1e-4 || v >= 1 - 1e-4) with v promoted to double,
// as the source compares it; NaN counts as invalid.  Valid values are positive floats, so their
// bit patterns order like the values: an exact radix select (11 + 11 + 10 bits, three passes) of
// the element of rank n / 2, which is what nth_element leaves at that index.  The histograms use
// integer atomics only, so the result does not depend on the order of execution.
static constexpr int kMedBins = 2048;

struct MedState {
    uint32_t prefix, rank, n, key;
};

struct MedMaps {
    const float* p[2];
    long long stride[2];  // floats per map
    int npx[2], c[2];
};

__device__ __forceinline__ bool med_valid(float v)
{
    const double w = (double)v;
    return !(w < 1e-4 || w >= 1 - 1e-4) && v == v;
}

__device__ __forceinline__ int med_shift(int pass) { return pass == 0 ? 21 : (pass == 1 ? 10 : 0); }

// grid (blocks, 2 * batch): blockIdx.y = b * 2 + map
__global__ void __launch_bounds__(kBlock) k_gmed_hist(MedMaps M, int pass,
                                                      const MedState* __restrict__ st,
                                                      uint32_t* __restrict__ hist)
{
    __shared__ uint32_t h[kMedBins];
    const int s = blockIdx.y, m = s & 1, b = s >> 1;
    for (int i = threadIdx.x; i < kMedBins; i += kBlock) h[i] = 0;
    __syncthreads();
    const float* p = M.p[m] + b * M.stride[m];
    const int c = M.c[m], n = M.npx[m];
    const int sh = med_shift(pass), psh = pass == 1 ? 21 : 10;
    const uint32_t msk = pass == 2 ? 0x3FFu : 0x7FFu;
    const uint32_t pre = pass > 0 ? st[s].prefix : 0u;
    const bool live = pass == 0 || st[s].n > 0;
    // A thread takes groups of four consecutive pixels and counts a run of equal bins in a
    // register, adding it to LDS when the bin changes (and once at the end): neighbouring depths
    // share their top digits, and 64 lanes adding to a handful of bins one by one would serialise.
    uint32_t run_bin = 0u, run_len = 0u;
    const int ngrp = (n + 3) / 4;
    for (int g = blockIdx.x * kBlock + threadIdx.x; live && g < ngrp; g += gridDim.x * kBlock) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int i = g * 4 + j;
            if (i >= n) break;
            const float v = p[(long long)i * c];
            if (!med_valid(v)) continue;
            const uint32_t k = __float_as_uint(v);
            if (pass > 0 && (k >> psh) != pre) continue;
            const uint32_t bin = (k >> sh) & msk;
            if (run_len && bin == run_bin) {
                ++run_len;
            } else {
                if (run_len) atomicAdd(&h[run_bin], run_len);
                run_bin = bin;
                run_len = 1u;
            }
        }
    }
    if (run_len) atomicAdd(&h[run_bin], run_len);
    __syncthreads();
    uint32_t* g = hist + (long long)s * kMedBins;
    for (int i = threadIdx.x; i < kMedBins; i += kBlock)
        if (h[i]) atomicAdd(&g[i], h[i]);
}

// One block per (panorama, map): the bin that holds the element of the remaining rank; the bins
// are cleared for the next pass.
__global__ void __launch_bounds__(kBlock) k_gmed_scan(int pass, uint32_t* __restrict__ hist,
                                                      MedState* __restrict__ st)
{
    constexpr int PER = kMedBins / kBlock;
    __shared__ uint32_t part[kBlock];
    const int s = blockIdx.x, t = threadIdx.x;
    uint32_t* g = hist + (long long)s * kMedBins;
    uint32_t loc[PER], sum = 0;
    for (int j = 0; j < PER; j++) {
        loc[j] = g[t * PER + j];
        sum += loc[j];
        g[t * PER + j] = 0u;
    }
    part[t] = sum;
    __syncthreads();
    for (int off = 1; off < kBlock; off <<= 1) {
        const uint32_t v = t >= off ? part[t - off] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    const uint32_t total = part[kBlock - 1];
    MedState S = st[s];
    if (pass == 0) {
        S.n = total;
        S.rank = total / 2;  // val0s.size() / 2, Depth.cpp:664-670
        S.prefix = 0;
        S.key = 0;
    }
    if (S.n == 0) {
        if (t == 0) st[s] = S;
        return;
    }
    const uint32_t excl = t ? part[t - 1] : 0u;
    if (S.rank >= excl && S.rank < part[t]) {
        uint32_t c = excl;
        for (int j = 0; j < PER; j++) {
            if (S.rank < c + loc[j]) {
                const uint32_t bin = t * PER + j;
                S.rank -= c;
                S.prefix = pass == 0 ? bin : ((S.prefix << (pass == 2 ? 10 : 11)) | bin);
                if (pass == 2) S.key = S.prefix;
                st[s] = S;
                break;
            }
            c += loc[j];
        }
    }
}

// scaling = m1 / m0 in fp32 on the valid pixels of map 0 (Depth.cpp:683-698).  A panorama with
// a map without any valid pixel: status 1, medians 0, nothing written.
__global__ void __launch_bounds__(kBlock) k_gmed_apply(float* __restrict__ map0, long long stride,
                                                       int npx, int c,
                                                       const MedState* __restrict__ st,
                                                       float* __restrict__ medians,
                                                       int* __restrict__ status)
{
    const int b = blockIdx.y;
    const MedState s0 = st[b * 2], s1 = st[b * 2 + 1];
    const bool ok = s0.n > 0 && s1.n > 0;
    const float m0 = ok ? __uint_as_float(s0.key) : 0.0f, m1 = ok ? __uint_as_float(s1.key) : 0.0f;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (medians) {
            medians[b * 2] = m0;
            medians[b * 2 + 1] = m1;
        }
        if (status) status[b] = ok ? 0 : 1;
    }
    if (!ok) return;
    const float scaling = m1 / m0;
    float* p = map0 + b * stride;
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < npx; i += gridDim.x * kBlock) {
        const float v = p[(long long)i * c];
        if (med_valid(v)) p[(long long)i * c] = v * scaling;
    }
}

size_t median_workspace_bytes(int batch)
{
    return (size_t)batch * 2 * (kMedBins * sizeof(uint32_t) + sizeof(MedState));
}

static unsigned stream_blocks(long long n)
{
    long long nb = (n + 4LL * kBlock - 1) / (4LL * kBlock);
    return (unsigned)(nb < 1 ? 1 : (nb > 512 ? 512 : nb));
}

void launch_median_scale(hipStream_t s, float* map0, int w0, int h0, int c0, const float* map1,
                         int w1, int h1, int c1, int batch, void* ws, float* medians, int* status)
{
    uint32_t* hist = (uint32_t*)ws;
    MedState* st = (MedState*)(hist + (size_t)batch * 2 * kMedBins);
    (void)hipMemsetAsync(ws, 0, median_workspace_bytes(batch), s);
    MedMaps M;
    M.p[0] = map0; M.p[1] = map1;
    M.npx[0] = w0 * h0; M.npx[1] = w1 * h1;
    M.c[0] = c0; M.c[1] = c1;
    M.stride[0] = (long long)w0 * h0 * c0; M.stride[1] = (long long)w1 * h1 * c1;
    const int nmax = M.npx[0] > M.npx[1] ? M.npx[0] : M.npx[1];
    const dim3 grid(stream_blocks(nmax), (unsigned)(2 * batch));
    for (int pass = 0; pass < 3; pass++) {
        hipLaunchKernelGGL(k_gmed_hist, grid, dim3(kBlock), 0, s, M, pass, st, hist);
        hipLaunchKernelGGL(k_gmed_scan, dim3((unsigned)(2 * batch)), dim3(kBlock), 0, s, pass,
                           hist, st);
    }
    hipLaunchKernelGGL(k_gmed_apply, dim3(stream_blocks(M.npx[0]), (unsigned)batch), dim3(kBlock),
                       0, s, map0, M.stride[0], M.npx[0], c0, st, medians, status);
}

// ---------------------------------------------------------------------------------------------
// CopyInvalidPixels: X = int((float)x * ratio_x), Y = int((float)y * ratio_y); channel 0 of the
// reference pixel is copied where it is < 1e-4 or >= 1 - 1e-4 (NaN compares false: not copied).
// An index that the float product pushes past the last column / row is clamped to it (the
// reference reads out of bounds there).
__global__ void __launch_bounds__(kBlock) k_copy_invalid(float* __restrict__ dst, int w, int h,
                                                         int c, const float* __restrict__ ref,
                                                         int rw, int rh, int rc, float ratio_x,
                                                         float ratio_y)
{
    const int b = blockIdx.y;
    const int n = w * h;
    float* d = dst + (long long)b * n * c;
    const float* r = ref + (long long)b * rw * rh * rc;
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        const int y = i / w, x = i - y * w;
        int X = (int)((float)x * ratio_x), Y = (int)((float)y * ratio_y);
        X = X < rw ? X : rw - 1;
        Y = Y < rh ? Y : rh - 1;
        const float v = r[((long long)Y * rw + X) * rc];
        const double wv = (double)v;
        if (wv < 1e-4 || wv >= 1 - 1e-4) d[(long long)i * c] = v;
    }
}

void launch_copy_invalid(hipStream_t s, float* dst, int w, int h, int c, const float* ref, int rw,
                         int rh, int rc, int batch)
{
    const float ratio_x = (float)rw / (float)w, ratio_y = (float)rh / (float)h;
    hipLaunchKernelGGL(k_copy_invalid, dim3(stream_blocks((long long)w * h), (unsigned)batch),
                       dim3(kBlock), 0, s, dst, w, h, c, ref, rw, rh, rc, ratio_x, ratio_y);
}

}  // namespace pf
