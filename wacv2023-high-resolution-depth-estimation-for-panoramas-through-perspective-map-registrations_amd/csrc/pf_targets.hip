// pf_targets.hip -- Laplacian-target scatter (Depth.cpp:1487-1647) as a two-stage gather.
//
// The projection of a fusion-grid point into a tile (SphericalTo2D + Value's truncation,
// Depth.cpp:111-118,168-182) depends only on the layout and the level, never on the panorama,
// and every grid point is a tap of up to five stencils.  So:
//
//  1. k_tapmap (once per layout and level, cached in the context): for every tile p and every
//     grid point of its box plus a one-pixel ring, the tile element index the reference's
//     Value() reads -- five correctly rounded divisions per point, done once instead of five
//     times per pixel and once per panorama.
//  2. targets_patch (per call; k_targets_multi runs it for every level in one launch): per
//     patch of band pixels and kTNB panoramas at a time, the covering tiles in index order (the
//     reference's single-thread accumulation); per tile the tap values of the patch plus a
//     one-pixel ring gathered through the map (+ the fused Depth2DepthTransform) into LDS, the
//     five-point sums in std::map key order, then the normalisation of Depth.cpp:1626-1647.
//     targets_wave (round 7, PF_TGT_WAVE=1, the default) is the same gather with one wave per
//     patch and the grid rows in registers instead of LDS; targets_patch stays for the validity
//     rule, the sharded partial sums and as the tests' reference.  targets_wave_weighted
//     (pf_fuse_weighted) is targets_wave with a weight per tap beside the value.
#include "pf_internal.hpp"

#include <cstdlib>

namespace pf {

__global__ void __launch_bounds__(256) k_tapmap(const TileGeom* __restrict__ geom,
                                                const TapBox* __restrict__ tb, int ntiles,
                                                const GridCol* __restrict__ cols,
                                                const GridRow* __restrict__ rows,
                                                int32_t* __restrict__ map)
{
    const int p = blockIdx.y;
    const TapBox B = tb[p];
    const long long n = (long long)B.nx * B.ny;
    const TileGeom g = geom[p];
    const long long lim = (long long)g.w * g.h * g.c;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n;
         i += (long long)gridDim.x * 256) {
        int yy = B.ymin + (int)(i / B.nx), xx = B.xmin + (int)(i % B.nx);
        const GridCol c = cols[xx + 1];
        const GridRow r = rows[yy + 1];
        float x, y;
        sph_to_2d(g, r.sz, r.cz, c.ca, c.sa, x, y);
        long long idx = tile_index(g, x, y);
        if (idx < 0) idx = 0;  // out-of-tile tap: the reference reads out of bounds; clamp
        if (idx >= lim) idx = lim - g.c;
        map[B.off + i] = (int32_t)idx;
    }
}

__device__ __forceinline__ bool in_box2(const TileBox& bx, int X, int Y)
{  // X runs x0, x0+xs, ... and stops before x1 (Depth.cpp:1565-1623)
    if (Y < bx.y0 || Y > bx.y1) return false;
    return bx.xs > 0 ? (X >= bx.x0 && X < bx.x1) : (X <= bx.x0 && X > bx.x1);
}

// ---------------------------------------------------------------------------------------------
// Layout audit (pf_layout_audit): k_tapmap's sibling.  Rows p < ntiles of the grid walk tile p's
// box and count, per pixel and tap of the five-point mask (the reference's visit order does not
// matter to a count), the taps whose projection leaves [0,1]^2 -- tested on the unclamped floats,
// Depth.cpp:1595 -- and the taps whose Value() index k_tapmap clamps.  Row p == ntiles walks the
// level's pixels and counts the covering tiles of each.  The flags are summed inside the wave
// (ballot + popcount, so the sums are wave-uniform), across the block's four waves through LDS,
// and leave the block as one atomic per counter; integer sums, so the result does not depend on
// the order the blocks arrive in.
// ctr: [0] taps outside, [1] taps clamped, [2] covered pixels, [3] uncovered interior pixels,
// [4] largest cover, [5] seam column covered; zeroed on the stream before the launch.
__device__ __forceinline__ unsigned long long wave_count(bool f)
{
    return (unsigned long long)__popcll(__ballot(f));
}

__global__ void __launch_bounds__(256) k_layout_audit(const TileGeom* __restrict__ geom,
                                                      const TileBox* __restrict__ box, int ntiles,
                                                      const GridCol* __restrict__ cols,
                                                      const GridRow* __restrict__ rows,
                                                      LevelDims L,
                                                      unsigned long long* __restrict__ ctr)
{
    __shared__ unsigned long long s_cnt[4][4];
    __shared__ int s_max[4], s_seam[4];
    const int p = blockIdx.y;
    unsigned long long outside = 0, clamped = 0, covered = 0, uncovered = 0;  // wave-uniform
    int seam = 0, most = 0;                                                   // per lane
    if (p < ntiles) {
        const TileBox bx = box[p];
        // X runs x0, x0+xs, ... and stops before x1 (in_box2): columns [xlo, xhi]
        const int xlo = bx.xs > 0 ? bx.x0 : bx.x1 + 1, xhi = bx.xs > 0 ? bx.x1 - 1 : bx.x0;
        const int nx = xhi - xlo + 1, ny = bx.y1 - bx.y0 + 1;
        const long long n = nx > 0 && ny > 0 ? (long long)nx * ny : 0;
        const TileGeom g = geom[p];
        const long long lim = (long long)g.w * g.h * g.c;
        for (long long i0 = (long long)blockIdx.x * 256; i0 < n; i0 += (long long)gridDim.x * 256) {
            const long long i = i0 + threadIdx.x;
            const bool live = i < n;
            const int Y = bx.y0 + (live ? (int)(i / nx) : 0), X = xlo + (live ? (int)(i % nx) : 0);
            const int dx[5] = {-1, 0, 0, 0, 1}, dy[5] = {0, -1, 0, 1, 0};
#pragma unroll
            for (int k = 0; k < 5; k++) {
                const GridCol c = cols[X + dx[k] + 1];
                const GridRow r = rows[Y + dy[k] + 1];
                float x, y;
                sph_to_2d(g, r.sz, r.cz, c.ca, c.sa, x, y);
                const long long idx = tile_index(g, x, y);
                outside += wave_count(live && (x < 0 || x > 1 || y < 0 || y > 1));
                clamped += wave_count(live && (idx < 0 || idx >= lim));
            }
        }
    } else {
        const long long n = (long long)L.w * L.h;
        for (long long i0 = (long long)blockIdx.x * 256; i0 < n; i0 += (long long)gridDim.x * 256) {
            const long long i = i0 + threadIdx.x;
            const bool live = i < n;
            const int Y = live ? (int)(i / L.w) : 0, X = live ? (int)(i % L.w) : 0;
            int cnt = 0;
            for (int q = 0; q < ntiles; q++) cnt += in_box2(box[q], X, Y) ? 1 : 0;
            covered += wave_count(live && cnt > 0);
            uncovered += wave_count(live && cnt == 0 && Y > L.h0 && Y < L.h1 && X >= 1);
            if (live && cnt > most) most = cnt;
            if (live && cnt > 0 && X == L.w - 1) seam = 1;
        }
    }
    for (int o = 32; o > 0; o >>= 1) most = max(most, __shfl_xor(most, o));
    const bool any_seam = __ballot(seam != 0) != 0;
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_cnt[wv][0] = outside;
        s_cnt[wv][1] = clamped;
        s_cnt[wv][2] = covered;
        s_cnt[wv][3] = uncovered;
        s_max[wv] = most;
        s_seam[wv] = any_seam ? 1 : 0;
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t < 4) {
        const unsigned long long v = s_cnt[0][t] + s_cnt[1][t] + s_cnt[2][t] + s_cnt[3][t];
        if (v) atomicAdd(&ctr[t], v);
    } else if (t == 4) {
        const int m = max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]));
        if (m) atomicMax(&ctr[4], (unsigned long long)m);
    } else if (t == 5) {
        if (s_seam[0] | s_seam[1] | s_seam[2] | s_seam[3]) atomicMax(&ctr[5], 1ull);
    }
}

// ---------------------------------------------------------------------------------------------
// Patch-staged gather.  Every fusion-grid point is a tap of up to five stencils, so gathering
// per pixel reads each tile value five times.  Here a block owns a kTPW x kTPH patch of band
// pixels and kTNB panoramas; for every tile whose box meets the patch (index order), the tap
// values of the patch plus a one-pixel ring are gathered once per grid point, transformed once
// (Depth2DepthTransform), staged in LDS, and the five-point stencils read LDS.
// patch height: 8 rows (2 pixels per thread) stages 1.29 grid points per pixel instead of 1.55
// at 4 rows; measured at C3 (profiles/r02 logs): 4 rows 0.687 ms, 8 rows 0.635, 16 rows 0.670
static constexpr int kTPW = 64, kTPH = 8;                        // patch of kTPW x kTPH pixels
static constexpr int kTPP = kTPW * kTPH / 256;                   // pixels per thread
static constexpr int kTGW = kTPW + 2, kTGH = kTPH + 2, kTG = kTGW * kTGH;  // grid points + ring
// panoramas per block: 4 / 16 measured 0.639-0.651 / 0.730 ms per C3 step against 0.618-0.623
// (profiles/r03/tgt)
static constexpr int kTNB = 8;

// One block's work: patch `pid` of level L for panoramas [bgrp*NB, +NB).
//
// MASK (pf_set_tile_validity, the *_valid kernels): an invalid tap -- its raw value fails the
// rule, or its transformed value is not finite -- is staged as NaN, and tile p contributes to a
// pixel of panorama q iff its five-point sum is not NaN, i.e. iff all five taps are valid (finite
// taps cannot sum to NaN: the partial sums may overflow to one infinity, never to both).  Coverage
// then depends on the data, so the count n is kept per panorama; the order of the tiles and the
// normalisation are the unmasked ones.  With MASK false this is the code it always was.
template <bool XFORM, int NB, bool MASK = false>
__device__ __forceinline__ void targets_patch(const TileGeom* __restrict__ geom,
                                              const TileBox* __restrict__ box,
                                              const TapBox* __restrict__ tb, int ntiles,
                                              const int32_t* __restrict__ map,
                                              const float* __restrict__ tiles, long long tstride,
                                              const float* __restrict__ coeffs, const LevelDims& L,
                                              int npx, int pid, int bgrp,
                                              float* __restrict__ lnorm, long long lstride,
                                              int batch, float (*sv)[kTG],
                                              const uint32_t* __restrict__ tmask, int nmw,
                                              float vlo = 0.0f, float vhi = 0.0f)
{
    const int X0 = (pid % npx) * kTPW, Y0 = L.h0 + (pid / npx) * kTPH;
    const int t = threadIdx.x;
    const int X = X0 + (t & (kTPW - 1));
    const int bbeg = bgrp * NB;
    float acc[kTPP][NB];
    int n[kTPP];
    int nq[kTPP][MASK ? NB : 1];  // MASK: the covering tiles per panorama
#pragma unroll
    for (int j = 0; j < kTPP; j++) {
        n[j] = 0;
#pragma unroll
        for (int q = 0; q < NB; q++) acc[j][q] = 0.0f;
        if constexpr (MASK) {
#pragma unroll
            for (int q = 0; q < NB; q++) nq[j][q] = 0;
        }
    }
    const int X1 = min(X0 + kTPW - 1, L.w - 1), Y1 = min(Y0 + kTPH - 1, L.h1);
    // one tile's contribution to the patch (tiles come in index order: the reference's
    // accumulation order); `last`: no staging follows, so no barrier after the stencils
    auto tile = [&](const int p, const bool last) {
        const TileBox bx = box[p];
        const TapBox B = tb[p];
        const long long toff = geom[p].off;
        float4 k[NB];
        if constexpr (XFORM) {
#pragma unroll
            for (int q = 0; q < NB; q++) {
                const int b = bbeg + q < batch ? bbeg + q : batch - 1;
                k[q] = *reinterpret_cast<const float4*>(coeffs + ((long long)b * ntiles + p) * 4);
            }
        }
        // stage the tap values of the patch + ring that lie in this tile's tap-index map
        for (int g = t; g < kTG; g += 256) {
            const int gx = X0 - 1 + g % kTGW - B.xmin, gy = Y0 - 1 + g / kTGW - B.ymin;
            if (gx < 0 || gx >= B.nx || gy < 0 || gy >= B.ny) continue;
            const int32_t m = map[B.off + (long long)gy * B.nx + gx];
            float v[NB];
#pragma unroll
            for (int q = 0; q < NB; q++) {
                const int b = bbeg + q < batch ? bbeg + q : batch - 1;
                v[q] = tiles[b * tstride + toff + m];
            }
#pragma unroll
            for (int q = 0; q < NB; q++) {
                float x = v[q];
                if constexpr (XFORM) x = cubic_map(x, k[q].x, k[q].y, k[q].z, k[q].w);
                if constexpr (MASK)
                    if (!(tile_ok(v[q], vlo, vhi) && isfinite(x))) x = __uint_as_float(0x7FC00000u);
                sv[q][g] = x;
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kTPP; j++) {
            const int r = t / kTPW + j * (256 / kTPW);  // row inside the patch
            const int Y = Y0 + r;
            if (X < L.w && Y <= L.h1 && Y > L.h0 && Y < L.h1 && in_box2(bx, X, Y)) {
                const int c = (r + 1) * kTGW + (t & (kTPW - 1)) + 1;  // (X, Y) in the grid
#pragma unroll
                for (int q = 0; q < NB; q++) {
                    // taps in std::map key order: (X-1,Y), (X,Y-1), (X,Y), (X,Y+1), (X+1,Y)
                    float Lp = 0;
                    Lp += sv[q][c - 1] * -0.25f;
                    Lp += sv[q][c - kTGW] * -0.25f;
                    Lp += sv[q][c] * 1.0f;
                    Lp += sv[q][c + kTGW] * -0.25f;
                    Lp += sv[q][c + 1] * -0.25f;
                    if constexpr (MASK) {
                        if (Lp == Lp) {
                            acc[j][q] += Lp;
                            nq[j][q]++;
                        }
                    } else {
                        acc[j][q] += Lp;
                    }
                }
                n[j]++;
            }
        }
        if (!last) __syncthreads();  // the next tile's staging overwrites sv
    };
    if (tmask) {  // the host's list of the tiles whose box meets this patch, as mask words
        int left = 0;  // tiles still to come (block-uniform)
        for (int w = 0; w < nmw; w++) left += __builtin_popcount(tmask[(long long)pid * nmw + w]);
        for (int w = 0; w < nmw; w++) {
            uint32_t m = tmask[(long long)pid * nmw + w];  // block-uniform
            while (m) {
                tile(w * 32 + __builtin_ctz(m), --left == 0);
                m &= m - 1;
            }
        }
    } else {
        for (int p = 0; p < ntiles; p++)
            if (box_meets(box[p], X0, X1, Y0, Y1)) tile(p, false);  // block-uniform
    }
#pragma unroll
    for (int j = 0; j < kTPP; j++) {
        const int Y = Y0 + t / kTPW + j * (256 / kTPW);
        if (!(X < L.w && Y <= L.h1)) continue;
        float scale = 1.0f;
        if (n[j] > 1) {
            float center = 0.0f;
            for (int i = 0; i < n[j]; i++) center += 1.0f;
            scale = 1.0f / center;
        }
        const long long o = (long long)Y * L.w + X;
#pragma unroll
        for (int q = 0; q < NB; q++) {
            const int b = bbeg + q;
            if (b >= batch) break;
            float out;
            if constexpr (MASK) {
                // 1 / center with center = 1 + 1 + ... (nq times) = (float)nq exactly
                const int m = nq[j][q];
                if (m == 0) out = __uint_as_float(PF_NAN_MARKER);
                else if (m == 1) out = acc[j][q];
                else out = acc[j][q] * (1.0f / (float)m);
            } else if (n[j] == 0) out = __uint_as_float(PF_NAN_MARKER);
            else if (n[j] == 1) out = acc[j][q];
            else out = acc[j][q] * scale;
            // nt: the planes' stores keep the tiles' lines in L2 for the neighbouring patches
            // (0.629-0.633 -> 0.618-0.623 ms per C3 step, profiles/r03/tgt)
            __builtin_nontemporal_store(out, &lnorm[b * lstride + o]);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Per-wave gather (round 7, PF_TGT_WAVE).  A kTPW = 64 column patch row is one wave wide, so a
// wave can own a whole patch: lane i holds column X0 + i of all kTGH grid rows in registers, the
// north / centre / south taps are the lane's own registers and the west / east taps are the
// neighbouring lanes' (DPP wave_shr:1 / wave_shl:1).  No LDS, no barrier; the four waves of a
// block are four independent work items.
//
// The ring columns X0 - 1 and X0 + 64 (the west tap of lane 0, the east tap of lane 63) of the
// kTPH patch rows are gathered by ONE extra load per tile and panorama: lane j < kTPH takes the
// west ring point of patch row j, lane kRingE + j the east one.  Row j's two ring values are
// read out of that register (v_readlane) into the `old` operand of the row's two DPP moves,
// which lane 0 / lane 63 keep (bound_ctrl off: a lane without a source lane keeps `old`).
// A grid point outside the tile's tap box takes the value of the box's nearest point; such a
// value only ever reaches pixels that in_box2 rejects.  The arithmetic per pixel is
// targets_patch's, operation for operation.
static constexpr int kRingE = 16;  // first lane of the east ring points
static_assert(kTPW == 64 && kTPH <= kRingE && kRingE + kTPH <= 64, "one wave per patch row");

__device__ __forceinline__ float dpp_west(float ring, float c)
{  // lane i <- lane i-1 (wave_shr:1), lane 0 <- ring
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(ring), __float_as_int(c),
                                                      0x138, 0xF, 0xF, false));
}
__device__ __forceinline__ float dpp_east(float ring, float c)
{  // lane i <- lane i+1 (wave_shl:1), lane 63 <- ring
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(ring), __float_as_int(c),
                                                      0x130, 0xF, 0xF, false));
}
__device__ __forceinline__ float lane_value(float v, int lane)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// One wave's work: patch `pid` of level L for panoramas [bgrp*NB, +NB), NP of them in flight.
template <bool XFORM, int NB>
__device__ __forceinline__ void targets_wave(const TileGeom* __restrict__ geom,
                                             const TileBox* __restrict__ box,
                                             const TapBox* __restrict__ tb, int ntiles,
                                             const int32_t* __restrict__ map,
                                             const float* __restrict__ tiles, long long tstride,
                                             const float* __restrict__ coeffs, const LevelDims& L,
                                             int npx, int pid, int bgrp,
                                             float* __restrict__ lnorm, long long lstride,
                                             int batch, const uint32_t* __restrict__ tmask, int nmw)
{
    constexpr int NP = NB < 2 ? NB : 2;  // panoramas in flight (the VGPR budget: DESIGN.md §3)
    static_assert(NB % NP == 0, "whole groups of panoramas in flight");
    const int X0 = (pid % npx) * kTPW, Y0 = L.h0 + (pid / npx) * kTPH;
    const int lane = threadIdx.x & 63;
    const int X = X0 + lane;
    const int bbeg = bgrp * NB;
    float acc[kTPH][NB];
#pragma unroll
    for (int j = 0; j < kTPH; j++) {
#pragma unroll
        for (int q = 0; q < NB; q++) acc[j][q] = 0.0f;
    }
    // bit j: tile bx covers this lane's pixel of patch row j
    auto covered = [&](const TileBox& bx) {
        uint32_t in = 0;
#pragma unroll
        for (int j = 0; j < kTPH; j++) {
            const int Y = Y0 + j;
            if (X < L.w && Y <= L.h1 && Y > L.h0 && Y < L.h1 && in_box2(bx, X, Y)) in |= 1u << j;
        }
        return in;
    };
    const int X1 = min(X0 + kTPW - 1, L.w - 1), Y1 = min(Y0 + kTPH - 1, L.h1);
    // The tap-map indices of tile p's grid, loaded once per tile for all NB panoramas.  A grid
    // point outside the tap box takes the nearest point of the box instead (no predicate, no
    // branch: every load is in bounds and the loads of a tile issue back to back).  They are kept
    // as 32-bit byte offsets into the panorama's tile: the launchers take this form only for tile
    // blocks of at most 2^30 elements, and the gathers need no 64-bit lane address.
    auto load_indices = [&](const int p, uint32_t (&mi)[kTGH], uint32_t& mr) {
        const TapBox B = tb[p];
        const int gx = max(min(X - B.xmin, B.nx - 1), 0);
#pragma unroll
        for (int r = 0; r < kTGH; r++) {
            const int gy = max(min(Y0 - 1 + r - B.ymin, B.ny - 1), 0);  // wave-uniform
            mi[r] = (uint32_t)map[B.off + (long long)gy * B.nx + gx] * 4u;
        }
        // this lane's ring point: patch row rj, column rX (the lanes outside the two runs load
        // one too, of a line the ring lanes load anyway)
        const bool reast = lane >= kRingE && lane < kRingE + kTPH;
        const int rj = reast ? lane - kRingE : lane < kTPH ? lane : 0;
        const int rX = reast ? X0 + kTPW : X0 - 1;
        const int rgx = max(min(rX - B.xmin, B.nx - 1), 0);
        const int rgy = max(min(Y0 + rj - B.ymin, B.ny - 1), 0);
        mr = (uint32_t)map[B.off + (long long)rgy * B.nx + rgx] * 4u;
    };
    // one tile's contribution (tiles come in index order: the reference's accumulation order)
    auto tile = [&](const int p) {
        uint32_t mi[kTGH], mr;
        load_indices(p, mi, mr);
        const long long toff = geom[p].off;
        // the pixels of this lane that the tile covers
        const uint32_t in = covered(box[p]);  // one register, not kTPH lane masks
#pragma unroll
        for (int q0 = 0; q0 < NB; q0 += NP) {
            float v[NP][kTGH], vr[NP];
#pragma unroll
            for (int u = 0; u < NP; u++) {
                const int b = bbeg + q0 + u < batch ? bbeg + q0 + u : batch - 1;
                const char* tv = reinterpret_cast<const char*>(tiles + b * tstride + toff);
#pragma unroll
                for (int r = 0; r < kTGH; r++) v[u][r] = *reinterpret_cast<const float*>(tv + mi[r]);
                vr[u] = *reinterpret_cast<const float*>(tv + mr);
            }
#pragma unroll
            for (int u = 0; u < NP; u++) {
                if constexpr (XFORM) {
                    const int b = bbeg + q0 + u < batch ? bbeg + q0 + u : batch - 1;
                    const float4 k =
                        *reinterpret_cast<const float4*>(coeffs + ((long long)b * ntiles + p) * 4);
#pragma unroll
                    for (int r = 0; r < kTGH; r++)
                        v[u][r] = cubic_map(v[u][r], k.x, k.y, k.z, k.w);
                    vr[u] = cubic_map(vr[u], k.x, k.y, k.z, k.w);
                }
#pragma unroll
                for (int j = 0; j < kTPH; j++) {
                    // every lane runs the DPP moves: a lane switched off is no source lane
                    const float W = dpp_west(lane_value(vr[u], j), v[u][j + 1]);
                    const float E = dpp_east(lane_value(vr[u], kRingE + j), v[u][j + 1]);
                    // taps in std::map key order: (X-1,Y), (X,Y-1), (X,Y), (X,Y+1), (X+1,Y)
                    float Lp = 0;
                    Lp += W * -0.25f;
                    Lp += v[u][j] * -0.25f;
                    Lp += v[u][j + 1] * 1.0f;
                    Lp += v[u][j + 2] * -0.25f;
                    Lp += E * -0.25f;
                    if (in & (1u << j)) acc[j][q0 + u] += Lp;
                }
            }
        }
    };
    // the tiles whose box meets this patch, as mask words: the host's list, or the box tests
    const int nw = (ntiles + 31) / 32;
    auto tile_word = [&](const int w) {
        uint32_t m = 0;  // wave-uniform
        if (tmask) {
            m = tmask[(long long)pid * nmw + w];
        } else {
            for (int p = w * 32; p < min(w * 32 + 32, ntiles); p++)
                if (box_meets(box[p], X0, X1, Y0, Y1)) m |= 1u << (p & 31);
        }
        return m;
    };
    for (int w = 0; w < nw; w++) {
        uint32_t m = tile_word(w);
        while (m) {
            tile(w * 32 + __builtin_ctz(m));
            m &= m - 1;
        }
    }
    // the covering tiles per pixel: counted over the same tiles afterwards, so the counts hold
    // no registers while the sums are gathered
    int n[kTPH];
#pragma unroll
    for (int j = 0; j < kTPH; j++) n[j] = 0;
    for (int w = 0; w < nw; w++) {
        uint32_t m = tile_word(w);
        while (m) {
            const uint32_t in = covered(box[w * 32 + __builtin_ctz(m)]);
#pragma unroll
            for (int j = 0; j < kTPH; j++) n[j] += (in >> j) & 1u;
            m &= m - 1;
        }
    }
#pragma unroll
    for (int j = 0; j < kTPH; j++) {
        const int Y = Y0 + j;
        if (!(X < L.w && Y <= L.h1)) continue;
        float scale = 1.0f;
        if (n[j] > 1) {
            float center = 0.0f;
            for (int i = 0; i < n[j]; i++) center += 1.0f;
            scale = 1.0f / center;
        }
        const long long o = (long long)Y * L.w + X;
#pragma unroll
        for (int q = 0; q < NB; q++) {
            const int b = bbeg + q;
            if (b >= batch) break;
            float out;
            if (n[j] == 0) out = __uint_as_float(PF_NAN_MARKER);
            else if (n[j] == 1) out = acc[j][q];
            else out = acc[j][q] * scale;
            __builtin_nontemporal_store(out, &lnorm[b * lstride + o]);
        }
    }
}

// The block form's kernels take the wave form with WAVE: a block is then four waves with four
// consecutive (patch, panorama group) work items, and the grid a quarter as many blocks.
template <bool XFORM, int NB, bool WAVE = false>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WAVE ? 4 : 1)))
k_targets_patch(const TileGeom* __restrict__ geom,
                                                       const TileBox* __restrict__ box,
                                                       const TapBox* __restrict__ tb, int ntiles,
                                                       const int32_t* __restrict__ map,
                                                       const float* __restrict__ tiles,
                                                       long long tstride,
                                                       const float* __restrict__ coeffs,
                                                       LevelDims L, int npx, int npatch,
                                                       float* __restrict__ lnorm,
                                                       long long lstride, int batch,
                                                       const uint32_t* __restrict__ tmask,
                                                       int nmw)
{
    // XCD-contiguous runs of patches (neighbouring patches read the same tile lines)
    const unsigned lb = xcd_remap(blockIdx.x, gridDim.x);
    if constexpr (WAVE) {
        const unsigned item =  // wave-uniform, and in scalar registers
            lb * 4u + (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
        if (item >= (unsigned)npatch * (unsigned)((batch + NB - 1) / NB)) return;
        targets_wave<XFORM, NB>(geom, box, tb, ntiles, map, tiles, tstride, coeffs, L, npx,
                                (int)(item % (unsigned)npatch), (int)(item / (unsigned)npatch), lnorm, lstride, batch,
                                tmask, nmw);
    } else {
        __shared__ float sv[NB][kTG];
        const int pid = (int)(lb % (unsigned)npatch), bgrp = (int)(lb / (unsigned)npatch);
        targets_patch<XFORM, NB>(geom, box, tb, ntiles, map, tiles, tstride, coeffs, L, npx, pid,
                                 bgrp, lnorm, lstride, batch, sv, tmask, nmw);
    }
}

// Every level's targets in ONE launch (round 4).  The per-level launches each streamed the
// tiles' lines from HBM: the coarse levels sample the same tile areas as the finest one, so the
// stage moved ~2x the tile bytes the finest level needs.  Here the blocks of all levels are
// ordered so that one region of the sphere is gathered at every level within a short window:
// per panorama group, the coarsest level's patch rows define zenith bands, and band by band the
// finest level's patches come first, then each coarser level's patches of the same band (a host
// table of (level, patch) entries).  The XCD-contiguous mapping gives every XCD a contiguous run
// of the table, so a band's lines are re-read from its L2 / the MALL instead of HBM.
// WAVE: the table is walked by waves, four consecutive entries per block, in the same order.
template <bool XFORM, int NB, bool WAVE = false>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WAVE ? 4 : 1)))
k_targets_multi(const TileGeom* __restrict__ geom,
                                                       int ntiles, const float* __restrict__ tiles,
                                                       long long tstride,
                                                       const float* __restrict__ coeffs,
                                                       TgtMulti M, const int2* __restrict__ order,
                                                       int batch)
{
    const unsigned lb = xcd_remap(blockIdx.x, gridDim.x);
    if constexpr (WAVE) {
        const unsigned item =  // wave-uniform, and in scalar registers
            lb * 4u + (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
        if (item >= (unsigned)M.nentries * (unsigned)((batch + NB - 1) / NB)) return;
        const int2 ent = order[item % (unsigned)M.nentries];  // (level, patch)
        const TgtLevel& T = M.lv[ent.x];
        targets_wave<XFORM, NB>(geom, T.box, T.tb, ntiles, T.map, tiles, tstride, coeffs, T.L,
                                T.npx, ent.y, (int)(item / (unsigned)M.nentries), T.lnorm, T.lstride, batch,
                                T.tmask, T.nmw);
    } else {
        __shared__ float sv[NB][kTG];
        const int e = (int)(lb % (unsigned)M.nentries), bgrp = (int)(lb / (unsigned)M.nentries);
        const int2 ent = order[e];  // (level, patch)
        const TgtLevel& T = M.lv[ent.x];
        targets_patch<XFORM, NB>(geom, T.box, T.tb, ntiles, T.map, tiles, tstride, coeffs, T.L,
                                 T.npx, ent.y, bgrp, T.lnorm, T.lstride, batch, sv, T.tmask, T.nmw);
    }
}

// The two gathers under the validity rule (MASK): the same blocks, tables and order.
template <bool XFORM, int NB>
__global__ void __launch_bounds__(256) k_targets_patch_valid(
    const TileGeom* __restrict__ geom, const TileBox* __restrict__ box,
    const TapBox* __restrict__ tb, int ntiles, const int32_t* __restrict__ map,
    const float* __restrict__ tiles, long long tstride, const float* __restrict__ coeffs,
    LevelDims L, int npx, int npatch, float* __restrict__ lnorm, long long lstride, int batch,
    const uint32_t* __restrict__ tmask, int nmw, float vlo, float vhi)
{
    __shared__ float sv[NB][kTG];
    const unsigned lb = xcd_remap(blockIdx.x, gridDim.x);
    const int pid = (int)(lb % (unsigned)npatch), bgrp = (int)(lb / (unsigned)npatch);
    targets_patch<XFORM, NB, true>(geom, box, tb, ntiles, map, tiles, tstride, coeffs, L, npx, pid,
                                   bgrp, lnorm, lstride, batch, sv, tmask, nmw, vlo, vhi);
}

template <bool XFORM, int NB>
__global__ void __launch_bounds__(256) k_targets_multi_valid(
    const TileGeom* __restrict__ geom, int ntiles, const float* __restrict__ tiles,
    long long tstride, const float* __restrict__ coeffs, TgtMulti M,
    const int2* __restrict__ order, int batch, float vlo, float vhi)
{
    __shared__ float sv[NB][kTG];
    const unsigned lb = xcd_remap(blockIdx.x, gridDim.x);
    const int e = (int)(lb % (unsigned)M.nentries), bgrp = (int)(lb / (unsigned)M.nentries);
    const int2 ent = order[e];  // (level, patch)
    const TgtLevel& T = M.lv[ent.x];
    targets_patch<XFORM, NB, true>(geom, T.box, T.tb, ntiles, T.map, tiles, tstride, coeffs, T.L,
                                   T.npx, ent.y, bgrp, T.lnorm, T.lstride, batch, sv, T.tmask,
                                   T.nmw, vlo, vhi);
}

// ---------------------------------------------------------------------------------------------
// Per-pixel tile weights (pf_fuse_weighted, pf_merge_weighted): targets_wave with a second plane.
// `weights` has the tiles' element layout (panorama b at weights + b * wstride; wstride 0: one set
// for the batch), so a tap's weight sits at the tap's own byte offset mi[r] / mr from a second
// base pointer.  Staging: the usable weight u(w) = w if 0 < w < +inf, else 0; the tap's value is a
// quiet NaN unless u(w) > 0 and its (transformed) value is finite.  Tile p contributes to a pixel
// iff its five-point sum Lp, formed as ever, is not NaN, with wmin = the smallest of the five
// staged weights (then > 0): acc = acc + wmin * Lp, ws = ws + wmin, a separate fp32 multiply and
// add, tiles in index order.  The pixel is acc * (1.0f / ws), or the marker when ws == 0.  With
// weights in {0, 1} that is targets_patch<MASK> under (-inf, +inf) bit for bit, and with every
// weight 1.0f it is targets_wave.
//
// Registers: the value rows and the weight rows of one panorama are in flight (NP = 1) and a wave
// owns kTWB = 4 panoramas (two accumulators per pixel and panorama): DESIGN.md section 12 has the
// compiler's count.  The weights of a shared set are loaded once per tile, not once per panorama.
static constexpr int kTWB = 4;

__device__ __forceinline__ float usable_weight(float w)
{
    return (0.0f < w && w < __uint_as_float(0x7F800000u)) ? w : 0.0f;
}

template <bool XFORM, int NB>
__device__ __forceinline__ void targets_wave_weighted(
    const TileGeom* __restrict__ geom, const TileBox* __restrict__ box,
    const TapBox* __restrict__ tb, int ntiles, const int32_t* __restrict__ map,
    const float* __restrict__ tiles, long long tstride, const float* __restrict__ weights,
    long long wstride, const float* __restrict__ coeffs, const LevelDims& L, int npx, int pid,
    int bgrp, float* __restrict__ lnorm, long long lstride, int batch,
    const uint32_t* __restrict__ tmask, int nmw)
{
    const int X0 = (pid % npx) * kTPW, Y0 = L.h0 + (pid / npx) * kTPH;
    const int lane = threadIdx.x & 63;
    const int X = X0 + lane;
    const int bbeg = bgrp * NB;
    float acc[kTPH][NB], ws[kTPH][NB];
#pragma unroll
    for (int j = 0; j < kTPH; j++) {
#pragma unroll
        for (int q = 0; q < NB; q++) acc[j][q] = ws[j][q] = 0.0f;
    }
    const int X1 = min(X0 + kTPW - 1, L.w - 1), Y1 = min(Y0 + kTPH - 1, L.h1);
    // one tile's contribution (tiles come in index order)
    auto tile = [&](const int p) {
        // the tap-map byte offsets of the tile's grid and of this lane's ring point, clamped to
        // the tap box as in targets_wave: shared by the value and the weight gathers
        uint32_t mi[kTGH], mr;
        {
            const TapBox B = tb[p];
            const int gx = max(min(X - B.xmin, B.nx - 1), 0);
#pragma unroll
            for (int r = 0; r < kTGH; r++) {
                const int gy = max(min(Y0 - 1 + r - B.ymin, B.ny - 1), 0);  // wave-uniform
                mi[r] = (uint32_t)map[B.off + (long long)gy * B.nx + gx] * 4u;
            }
            const bool reast = lane >= kRingE && lane < kRingE + kTPH;
            const int rj = reast ? lane - kRingE : lane < kTPH ? lane : 0;
            const int rX = reast ? X0 + kTPW : X0 - 1;
            const int rgx = max(min(rX - B.xmin, B.nx - 1), 0);
            const int rgy = max(min(Y0 + rj - B.ymin, B.ny - 1), 0);
            mr = (uint32_t)map[B.off + (long long)rgy * B.nx + rgx] * 4u;
        }
        const long long toff = geom[p].off;
        const TileBox bx = box[p];
        uint32_t in = 0;  // bit j: the tile covers this lane's pixel of patch row j
#pragma unroll
        for (int j = 0; j < kTPH; j++) {
            const int Y = Y0 + j;
            if (X < L.w && Y <= L.h1 && Y > L.h0 && Y < L.h1 && in_box2(bx, X, Y)) in |= 1u << j;
        }
        float w[kTGH], wr;
        auto load_weights = [&](const int b) {
            const char* wv = reinterpret_cast<const char*>(weights + b * wstride + toff);
#pragma unroll
            for (int r = 0; r < kTGH; r++)
                w[r] = usable_weight(*reinterpret_cast<const float*>(wv + mi[r]));
            wr = usable_weight(*reinterpret_cast<const float*>(wv + mr));
        };
        if (wstride == 0) load_weights(0);  // wave-uniform
#pragma unroll
        for (int q = 0; q < NB; q++) {
            const int b = bbeg + q < batch ? bbeg + q : batch - 1;
            const char* tv = reinterpret_cast<const char*>(tiles + b * tstride + toff);
            float v[kTGH], vr;
#pragma unroll
            for (int r = 0; r < kTGH; r++) v[r] = *reinterpret_cast<const float*>(tv + mi[r]);
            vr = *reinterpret_cast<const float*>(tv + mr);
            if (wstride != 0) load_weights(b);
            if constexpr (XFORM) {
                const float4 k =
                    *reinterpret_cast<const float4*>(coeffs + ((long long)b * ntiles + p) * 4);
#pragma unroll
                for (int r = 0; r < kTGH; r++) v[r] = cubic_map(v[r], k.x, k.y, k.z, k.w);
                vr = cubic_map(vr, k.x, k.y, k.z, k.w);
            }
            const float qnan = __uint_as_float(0x7FC00000u);
#pragma unroll
            for (int r = 0; r < kTGH; r++)
                if (!(w[r] > 0.0f && isfinite(v[r]))) v[r] = qnan;
            if (!(wr > 0.0f && isfinite(vr))) vr = qnan;
#pragma unroll
            for (int j = 0; j < kTPH; j++) {
                // every lane runs the DPP moves: a lane switched off is no source lane
                const float W = dpp_west(lane_value(vr, j), v[j + 1]);
                const float E = dpp_east(lane_value(vr, kRingE + j), v[j + 1]);
                const float wW = dpp_west(lane_value(wr, j), w[j + 1]);
                const float wE = dpp_east(lane_value(wr, kRingE + j), w[j + 1]);
                // taps in std::map key order: (X-1,Y), (X,Y-1), (X,Y), (X,Y+1), (X+1,Y)
                float Lp = 0;
                Lp += W * -0.25f;
                Lp += v[j] * -0.25f;
                Lp += v[j + 1] * 1.0f;
                Lp += v[j + 2] * -0.25f;
                Lp += E * -0.25f;
                const float wmin = fminf(fminf(fminf(wW, w[j]), fminf(w[j + 1], w[j + 2])), wE);
                if ((in & (1u << j)) && Lp == Lp) {
                    acc[j][q] = acc[j][q] + wmin * Lp;
                    ws[j][q] = ws[j][q] + wmin;
                }
            }
        }
    };
    // the tiles whose box meets this patch, as mask words: the host's list, or the box tests
    const int nw = (ntiles + 31) / 32;
    for (int wd = 0; wd < nw; wd++) {
        uint32_t m = 0;  // wave-uniform
        if (tmask) {
            m = tmask[(long long)pid * nmw + wd];
        } else {
            for (int p = wd * 32; p < min(wd * 32 + 32, ntiles); p++)
                if (box_meets(box[p], X0, X1, Y0, Y1)) m |= 1u << (p & 31);
        }
        while (m) {
            tile(wd * 32 + __builtin_ctz(m));
            m &= m - 1;
        }
    }
#pragma unroll
    for (int j = 0; j < kTPH; j++) {
        const int Y = Y0 + j;
        if (!(X < L.w && Y <= L.h1)) continue;
        const long long o = (long long)Y * L.w + X;
#pragma unroll
        for (int q = 0; q < NB; q++) {
            const int b = bbeg + q;
            if (b >= batch) break;
            const float out = ws[j][q] == 0.0f ? __uint_as_float(PF_NAN_MARKER)
                                               : acc[j][q] * (1.0f / ws[j][q]);
            __builtin_nontemporal_store(out, &lnorm[b * lstride + o]);
        }
    }
}

// The weighted gather of one level (k_targets_patch's wave form) and of every level in one launch
// (k_targets_multi's): the same work items, tables and order.
template <bool XFORM, int NB>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4)))
k_targets_patch_weighted(const TileGeom* __restrict__ geom, const TileBox* __restrict__ box,
                         const TapBox* __restrict__ tb, int ntiles,
                         const int32_t* __restrict__ map, const float* __restrict__ tiles,
                         long long tstride, const float* __restrict__ weights, long long wstride,
                         const float* __restrict__ coeffs, LevelDims L, int npx, int npatch,
                         float* __restrict__ lnorm, long long lstride, int batch,
                         const uint32_t* __restrict__ tmask, int nmw)
{
    const unsigned lb = xcd_remap(blockIdx.x, gridDim.x);
    const unsigned item =  // wave-uniform, and in scalar registers
        lb * 4u + (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (item >= (unsigned)npatch * (unsigned)((batch + NB - 1) / NB)) return;
    targets_wave_weighted<XFORM, NB>(geom, box, tb, ntiles, map, tiles, tstride, weights, wstride,
                                     coeffs, L, npx, (int)(item % (unsigned)npatch),
                                     (int)(item / (unsigned)npatch), lnorm, lstride, batch, tmask,
                                     nmw);
}

template <bool XFORM, int NB>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4)))
k_targets_multi_weighted(const TileGeom* __restrict__ geom, int ntiles,
                         const float* __restrict__ tiles, long long tstride,
                         const float* __restrict__ weights, long long wstride,
                         const float* __restrict__ coeffs, TgtMulti M,
                         const int2* __restrict__ order, int batch)
{
    const unsigned lb = xcd_remap(blockIdx.x, gridDim.x);
    const unsigned item =  // wave-uniform, and in scalar registers
        lb * 4u + (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (item >= (unsigned)M.nentries * (unsigned)((batch + NB - 1) / NB)) return;
    const int2 ent = order[item % (unsigned)M.nentries];  // (level, patch)
    const TgtLevel& T = M.lv[ent.x];
    targets_wave_weighted<XFORM, NB>(geom, T.box, T.tb, ntiles, T.map, tiles, tstride, weights,
                                     wstride, coeffs, T.L, T.npx, ent.y,
                                     (int)(item / (unsigned)M.nentries), T.lnorm, T.lstride, batch,
                                     T.tmask, T.nmw);
}

// PF_TGT_WAVE (read per call): 1 = the per-wave gather, 0 = the block form.  The validity-rule
// kernels and k_targets_patch_partial have the block form only, and so have layouts of more than
// 2^30 tile elements per panorama.
static constexpr int kTgtWaveDefault = 1;
static bool targets_wave_on(long long tstride)
{
    if (tstride > (1ll << 30)) return false;  // targets_wave's 32-bit byte offsets into a tile
    const char* e = getenv("PF_TGT_WAVE");
    return (e && *e ? atoi(e) : kTgtWaveDefault) != 0;
}

int targets_patch_w() { return kTPW; }
int targets_patch_h() { return kTPH; }
int targets_batch() { return kTNB; }

void launch_targets_multi(hipStream_t s, const TileGeom* geom, int ntiles, const float* tiles,
                          long long tstride, const float* coeffs, const TgtMulti& M,
                          const int2* order, int batch, TileValid tv)
{
    // one panorama (pf_merge, C2 / C5): blocks of one panorama, not kTNB copies of it
    const int nb = batch == 1 ? 1 : kTNB;
    const dim3 g((unsigned)((long long)M.nentries * ((batch + nb - 1) / nb)));
    if (tv.on) {
        if (nb == 1 && coeffs)
            hipLaunchKernelGGL((k_targets_multi_valid<true, 1>), g, dim3(256), 0, s, geom, ntiles,
                               tiles, tstride, coeffs, M, order, batch, tv.lo, tv.hi);
        else if (nb == 1)
            hipLaunchKernelGGL((k_targets_multi_valid<false, 1>), g, dim3(256), 0, s, geom, ntiles,
                               tiles, tstride, coeffs, M, order, batch, tv.lo, tv.hi);
        else if (coeffs)
            hipLaunchKernelGGL((k_targets_multi_valid<true, kTNB>), g, dim3(256), 0, s, geom,
                               ntiles, tiles, tstride, coeffs, M, order, batch, tv.lo, tv.hi);
        else
            hipLaunchKernelGGL((k_targets_multi_valid<false, kTNB>), g, dim3(256), 0, s, geom,
                               ntiles, tiles, tstride, coeffs, M, order, batch, tv.lo, tv.hi);
        return;
    }
    if (targets_wave_on(tstride)) {  // four work items (one per wave) to the block
        const dim3 gw((g.x + 3) / 4);
        if (nb == 1 && coeffs)
            hipLaunchKernelGGL((k_targets_multi<true, 1, true>), gw, dim3(256), 0, s, geom, ntiles,
                               tiles, tstride, coeffs, M, order, batch);
        else if (nb == 1)
            hipLaunchKernelGGL((k_targets_multi<false, 1, true>), gw, dim3(256), 0, s, geom,
                               ntiles, tiles, tstride, coeffs, M, order, batch);
        else if (coeffs)
            hipLaunchKernelGGL((k_targets_multi<true, kTNB, true>), gw, dim3(256), 0, s, geom,
                               ntiles, tiles, tstride, coeffs, M, order, batch);
        else
            hipLaunchKernelGGL((k_targets_multi<false, kTNB, true>), gw, dim3(256), 0, s, geom,
                               ntiles, tiles, tstride, coeffs, M, order, batch);
        return;
    }
    if (nb == 1 && coeffs)
        hipLaunchKernelGGL((k_targets_multi<true, 1>), g, dim3(256), 0, s, geom, ntiles, tiles,
                           tstride, coeffs, M, order, batch);
    else if (nb == 1)
        hipLaunchKernelGGL((k_targets_multi<false, 1>), g, dim3(256), 0, s, geom, ntiles, tiles,
                           tstride, coeffs, M, order, batch);
    else if (coeffs)
        hipLaunchKernelGGL((k_targets_multi<true, kTNB>), g, dim3(256), 0, s, geom, ntiles, tiles,
                           tstride, coeffs, M, order, batch);
    else
        hipLaunchKernelGGL((k_targets_multi<false, kTNB>), g, dim3(256), 0, s, geom, ntiles,
                           tiles, tstride, coeffs, M, order, batch);
}

void launch_targets_patch(hipStream_t s, const TileGeom* geom, const TileBox* box,
                          const TapBox* tb, int ntiles, const int32_t* map, const float* tiles,
                          long long tstride, const float* coeffs, LevelDims L, float* lnorm,
                          long long lstride, int batch, const uint32_t* tmask, int nmw,
                          TileValid tv)
{
    const int npx = (L.w + kTPW - 1) / kTPW;
    const int npy = (L.h1 - L.h0 + 1 + kTPH - 1) / kTPH;
    const int npatch = npx * npy;
    const int nb = batch == 1 ? 1 : kTNB;
    const dim3 g((unsigned)((long long)npatch * ((batch + nb - 1) / nb)));
    if (tv.on) {
        if (nb == 1 && coeffs)
            hipLaunchKernelGGL((k_targets_patch_valid<true, 1>), g, dim3(256), 0, s, geom, box, tb,
                               ntiles, map, tiles, tstride, coeffs, L, npx, npatch, lnorm, lstride,
                               batch, tmask, nmw, tv.lo, tv.hi);
        else if (nb == 1)
            hipLaunchKernelGGL((k_targets_patch_valid<false, 1>), g, dim3(256), 0, s, geom, box,
                               tb, ntiles, map, tiles, tstride, coeffs, L, npx, npatch, lnorm,
                               lstride, batch, tmask, nmw, tv.lo, tv.hi);
        else if (coeffs)
            hipLaunchKernelGGL((k_targets_patch_valid<true, kTNB>), g, dim3(256), 0, s, geom, box,
                               tb, ntiles, map, tiles, tstride, coeffs, L, npx, npatch, lnorm,
                               lstride, batch, tmask, nmw, tv.lo, tv.hi);
        else
            hipLaunchKernelGGL((k_targets_patch_valid<false, kTNB>), g, dim3(256), 0, s, geom, box,
                               tb, ntiles, map, tiles, tstride, coeffs, L, npx, npatch, lnorm,
                               lstride, batch, tmask, nmw, tv.lo, tv.hi);
        return;
    }
    if (targets_wave_on(tstride)) {  // four work items (one per wave) to the block
        const dim3 gw((g.x + 3) / 4);
        if (nb == 1 && coeffs)
            hipLaunchKernelGGL((k_targets_patch<true, 1, true>), gw, dim3(256), 0, s, geom, box, tb,
                               ntiles, map, tiles, tstride, coeffs, L, npx, npatch, lnorm, lstride,
                               batch, tmask, nmw);
        else if (nb == 1)
            hipLaunchKernelGGL((k_targets_patch<false, 1, true>), gw, dim3(256), 0, s, geom, box,
                               tb, ntiles, map, tiles, tstride, coeffs, L, npx, npatch, lnorm,
                               lstride, batch, tmask, nmw);
        else if (coeffs)
            hipLaunchKernelGGL((k_targets_patch<true, kTNB, true>), gw, dim3(256), 0, s, geom, box,
                               tb, ntiles, map, tiles, tstride, coeffs, L, npx, npatch, lnorm,
                               lstride, batch, tmask, nmw);
        else
            hipLaunchKernelGGL((k_targets_patch<false, kTNB, true>), gw, dim3(256), 0, s, geom,
                               box, tb, ntiles, map, tiles, tstride, coeffs, L, npx, npatch, lnorm,
                               lstride, batch, tmask, nmw);
        return;
    }
    if (nb == 1 && coeffs)
        hipLaunchKernelGGL((k_targets_patch<true, 1>), g, dim3(256), 0, s, geom, box, tb, ntiles,
                           map, tiles, tstride, coeffs, L, npx, npatch, lnorm, lstride, batch,
                           tmask, nmw);
    else if (nb == 1)
        hipLaunchKernelGGL((k_targets_patch<false, 1>), g, dim3(256), 0, s, geom, box, tb, ntiles,
                           map, tiles, tstride, coeffs, L, npx, npatch, lnorm, lstride, batch,
                           tmask, nmw);
    else if (coeffs)
        hipLaunchKernelGGL((k_targets_patch<true, kTNB>), g, dim3(256), 0, s, geom, box, tb,
                           ntiles, map, tiles, tstride, coeffs, L, npx, npatch, lnorm, lstride,
                           batch, tmask, nmw);
    else
        hipLaunchKernelGGL((k_targets_patch<false, kTNB>), g, dim3(256), 0, s, geom, box, tb,
                           ntiles, map, tiles, tstride, coeffs, L, npx, npatch, lnorm, lstride,
                           batch, tmask, nmw);
}

// The weighted gathers have the wave form only: the callers refuse layouts of more than 2^30 tile
// elements per panorama (targets_weighted_max_elems).
long long targets_weighted_max_elems() { return 1ll << 30; }

void launch_targets_multi_weighted(hipStream_t s, const TileGeom* geom, int ntiles,
                                   const float* tiles, long long tstride, const float* weights,
                                   long long wstride, const float* coeffs, const TgtMulti& M,
                                   const int2* order, int batch)
{
    const int nb = batch == 1 ? 1 : kTWB;
    const dim3 gw((unsigned)(((long long)M.nentries * ((batch + nb - 1) / nb) + 3) / 4));
    if (nb == 1 && coeffs)
        hipLaunchKernelGGL((k_targets_multi_weighted<true, 1>), gw, dim3(256), 0, s, geom, ntiles,
                           tiles, tstride, weights, wstride, coeffs, M, order, batch);
    else if (nb == 1)
        hipLaunchKernelGGL((k_targets_multi_weighted<false, 1>), gw, dim3(256), 0, s, geom, ntiles,
                           tiles, tstride, weights, wstride, coeffs, M, order, batch);
    else if (coeffs)
        hipLaunchKernelGGL((k_targets_multi_weighted<true, kTWB>), gw, dim3(256), 0, s, geom,
                           ntiles, tiles, tstride, weights, wstride, coeffs, M, order, batch);
    else
        hipLaunchKernelGGL((k_targets_multi_weighted<false, kTWB>), gw, dim3(256), 0, s, geom,
                           ntiles, tiles, tstride, weights, wstride, coeffs, M, order, batch);
}

void launch_targets_patch_weighted(hipStream_t s, const TileGeom* geom, const TileBox* box,
                                   const TapBox* tb, int ntiles, const int32_t* map,
                                   const float* tiles, long long tstride, const float* weights,
                                   long long wstride, const float* coeffs, LevelDims L,
                                   float* lnorm, long long lstride, int batch,
                                   const uint32_t* tmask, int nmw)
{
    const int npx = (L.w + kTPW - 1) / kTPW;
    const int npy = (L.h1 - L.h0 + 1 + kTPH - 1) / kTPH;
    const int npatch = npx * npy;
    const int nb = batch == 1 ? 1 : kTWB;
    const dim3 gw((unsigned)(((long long)npatch * ((batch + nb - 1) / nb) + 3) / 4));
    if (nb == 1 && coeffs)
        hipLaunchKernelGGL((k_targets_patch_weighted<true, 1>), gw, dim3(256), 0, s, geom, box, tb,
                           ntiles, map, tiles, tstride, weights, wstride, coeffs, L, npx, npatch,
                           lnorm, lstride, batch, tmask, nmw);
    else if (nb == 1)
        hipLaunchKernelGGL((k_targets_patch_weighted<false, 1>), gw, dim3(256), 0, s, geom, box,
                           tb, ntiles, map, tiles, tstride, weights, wstride, coeffs, L, npx,
                           npatch, lnorm, lstride, batch, tmask, nmw);
    else if (coeffs)
        hipLaunchKernelGGL((k_targets_patch_weighted<true, kTWB>), gw, dim3(256), 0, s, geom, box,
                           tb, ntiles, map, tiles, tstride, weights, wstride, coeffs, L, npx,
                           npatch, lnorm, lstride, batch, tmask, nmw);
    else
        hipLaunchKernelGGL((k_targets_patch_weighted<false, kTWB>), gw, dim3(256), 0, s, geom, box,
                           tb, ntiles, map, tiles, tstride, weights, wstride, coeffs, L, npx,
                           npatch, lnorm, lstride, batch, tmask, nmw);
}

void launch_layout_audit(hipStream_t s, const TileGeom* geom, const TileBox* box, int ntiles,
                         const GridCol* cols, const GridRow* rows, LevelDims L,
                         unsigned long long* ctr)
{
    // the widest row of the grid is the coverage row: the level's w * h pixels
    long long nb = ((long long)L.w * L.h + 255) / 256;
    if (nb > 4096) nb = 4096;
    if (nb < 1) nb = 1;
    dim3 grid((unsigned)nb, ntiles + 1);
    hipLaunchKernelGGL(k_layout_audit, grid, dim3(256), 0, s, geom, box, ntiles, cols, rows, L,
                       ctr);
}

void launch_tapmap(hipStream_t s, const TileGeom* geom, const TapBox* tb, int ntiles,
                   long long max_points, const GridCol* cols, const GridRow* rows, int32_t* map)
{
    long long nb = (max_points + 255) / 256;
    if (nb > 4096) nb = 4096;
    if (nb < 1) nb = 1;
    dim3 grid((unsigned)nb, ntiles);
    hipLaunchKernelGGL(k_tapmap, grid, dim3(256), 0, s, geom, tb, ntiles, cols, rows, map);
}

// Partial sums of tiles [t0, t1) for one panorama on rows [r0, r1) of the band (pf_fuse_partial,
// pf_fuse_partial_rows: the sharded fusion): lsum = the tiles' Laplacians added in tile order,
// cnt = how many, with targets_patch's per-pixel arithmetic.  Staged like targets_patch, for one
// panorama: a block owns one patch of the level's targets grid (kTPW x kTPH from row h0, the
// grid of the host's per-patch tile masks) and, for every tile of the range whose box meets the
// patch (the mask words ANDed with the range, index order), gathers the tap values of the patch
// plus a one-pixel ring once from the tap-index map, transforms them once
// (Depth2DepthTransform), stages them in LDS and reads the five-point stencils from LDS.  The
// launch covers the grid's patch rows that meet [r0, r1).  The per-pixel gather form re-read
// every tile value five times and tested all t1-t0 boxes per pixel: C5 at world 1 spent 1.17 ms
// per panorama in it, against 0.55 ms for the one-call path's k_targets_multi.
template <bool XFORM>
__global__ void __launch_bounds__(256) k_targets_patch_partial(const TileGeom* __restrict__ geom,
                                                               const TileBox* __restrict__ box,
                                                               const TapBox* __restrict__ tb,
                                                               const uint32_t* __restrict__ tmask,
                                                               int nmw, int t0, int t1,
                                                               const int32_t* __restrict__ map,
                                                               const float* __restrict__ tiles,
                                                               const float* __restrict__ coeffs,
                                                               LevelDims L, float* __restrict__ lsum,
                                                               float* __restrict__ cnt, int r0,
                                                               int r1, int npx, int py0)
{
    __shared__ float sv[kTG];
    const unsigned lb = xcd_remap(blockIdx.x, gridDim.x);
    const int px = (int)(lb % (unsigned)npx), py = py0 + (int)(lb / (unsigned)npx);
    const int pid = py * npx + px;
    const int X0 = px * kTPW, Y0 = L.h0 + py * kTPH;
    const int t = threadIdx.x;
    const int X = X0 + (t & (kTPW - 1));
    const int X1 = min(X0 + kTPW - 1, L.w - 1);
    // rows of the patch in [r0, r1) where Depth.cpp has targets (h0 < Y < h1)
    const int ya = max(max(Y0, r0), L.h0 + 1), yb = min(min(Y0 + kTPH - 1, r1 - 1), L.h1 - 1);
    float acc[kTPP], n[kTPP];
#pragma unroll
    for (int j = 0; j < kTPP; j++) acc[j] = n[j] = 0.0f;
    auto tile = [&](const int p) {
        const TileBox bx = box[p];
        const TapBox B = tb[p];
        const float* tv = tiles + geom[p].off;
        float4 k = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (XFORM) k = *reinterpret_cast<const float4*>(coeffs + (long long)p * 4);
        for (int g = t; g < kTG; g += 256) {
            const int gx = X0 - 1 + g % kTGW - B.xmin, gy = Y0 - 1 + g / kTGW - B.ymin;
            if (gx < 0 || gx >= B.nx || gy < 0 || gy >= B.ny) continue;
            float x = tv[map[B.off + (long long)gy * B.nx + gx]];
            if constexpr (XFORM) x = cubic_map(x, k.x, k.y, k.z, k.w);
            sv[g] = x;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kTPP; j++) {
            const int r = t / kTPW + j * (256 / kTPW);
            const int Y = Y0 + r;
            if (X <= X1 && Y >= ya && Y <= yb && in_box2(bx, X, Y)) {
                const int c = (r + 1) * kTGW + (t & (kTPW - 1)) + 1;
                // taps in std::map key order: (X-1,Y), (X,Y-1), (X,Y), (X,Y+1), (X+1,Y)
                float Lp = 0;
                Lp += sv[c - 1] * -0.25f;
                Lp += sv[c - kTGW] * -0.25f;
                Lp += sv[c] * 1.0f;
                Lp += sv[c + kTGW] * -0.25f;
                Lp += sv[c + 1] * -0.25f;
                acc[j] += Lp;
                n[j] += 1.0f;
            }
        }
        __syncthreads();
    };
    if (ya <= yb && t0 < t1) {
        for (int w = t0 >> 5; w <= (t1 - 1) >> 5; w++) {
            const int lo = max(t0 - 32 * w, 0), hi = min(t1 - 32 * w, 32);
            const uint32_t range = (hi >= 32 ? 0xFFFFFFFFu : ((1u << hi) - 1u)) & ~((1u << lo) - 1u);
            uint32_t m = tmask[(long long)pid * nmw + w] & range;  // block-uniform
            while (m) {
                tile(w * 32 + __builtin_ctz(m));
                m &= m - 1;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < kTPP; j++) {
        const int Y = Y0 + t / kTPW + j * (256 / kTPW);
        if (X > X1 || Y < r0 || Y >= r1 || Y > L.h1) continue;
        const long long o = (long long)Y * L.w + X;
        lsum[o] = acc[j];
        cnt[o] = n[j];
    }
}

hipError_t launch_targets_partial(hipStream_t s, const TileGeom* geom, const TileBox* box,
                                const TapBox* tb, const uint32_t* tmask, int nmw, int t0, int t1,
                                const int32_t* map, const float* tiles, const float* coeffs,
                                LevelDims L, float* lsum, float* cnt, int r0, int r1)
{
    if (r1 <= r0 || L.w <= 0) return hipSuccess;
    // rows of [r0, r1) outside the band [h0, h1]: no targets (zero sums and counts)
    const size_t rowb = sizeof(float) * (size_t)L.w;
    const int za = r0, zb = min(r1, L.h0);
    hipError_t e = hipSuccess;
    if (zb > za) {
        if (e == hipSuccess) e = hipMemsetAsync(lsum + (size_t)za * L.w, 0, rowb * (zb - za), s);
        if (e == hipSuccess) e = hipMemsetAsync(cnt + (size_t)za * L.w, 0, rowb * (zb - za), s);
    }
    const int wa = max(r0, L.h1 + 1), wb = r1;
    if (wb > wa) {
        if (e == hipSuccess) e = hipMemsetAsync(lsum + (size_t)wa * L.w, 0, rowb * (wb - wa), s);
        if (e == hipSuccess) e = hipMemsetAsync(cnt + (size_t)wa * L.w, 0, rowb * (wb - wa), s);
    }
    const int ba = max(r0, L.h0), bb = min(r1, L.h1 + 1);  // band rows of the range
    if (e != hipSuccess || bb <= ba) return e;
    const int npx = (L.w + kTPW - 1) / kTPW;
    const int py0 = (ba - L.h0) / kTPH, py1 = (bb - 1 - L.h0) / kTPH;
    const unsigned g = (unsigned)npx * (unsigned)(py1 - py0 + 1);
    if (coeffs)
        hipLaunchKernelGGL(k_targets_patch_partial<true>, dim3(g), dim3(256), 0, s, geom, box, tb,
                           tmask, nmw, t0, t1, map, tiles, coeffs, L, lsum, cnt, r0, r1, npx, py0);
    else
        hipLaunchKernelGGL(k_targets_patch_partial<false>, dim3(g), dim3(256), 0, s, geom, box, tb,
                           tmask, nmw, t0, t1, map, tiles, coeffs, L, lsum, cnt, r0, r1, npx, py0);
    return hipGetLastError();
}

}  // namespace pf
