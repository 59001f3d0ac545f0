// pf_consist.hip -- overlap-consistent tile registration: the tile-pair overlap table
// (k_paircount, k_pairidx), the pair moment sums (k_pair_moments), the joint normal equations of
// all tiles of a panorama assembled and solved by a Cholesky factorisation (k_consist_solve), and
// the overlap statistics of a set of coefficients (k_overlap_stats).
//
// E(c) = sum_p sum_{s in S_p} (u_s.c_p - y_s)^2 + lambda sum_{(p,q)} sum_{s in O_pq} (u_s.c_p - v_s.c_q)^2
// with u = (X^3, X^2, X, 1) of tile p's value and v the same row of tile q's value at the sample's
// grid direction.  O_pq: the registration samples of tile p whose direction lies inside tile q's
// window (den > 0, 0 <= x <= 1, 0 <= y <= 1 in fp32, no clamping).  Every sum is taken in
// k_register's order (lane l of 256 adds samples l, l + 256, ... from 0.0, then the halving tree),
// every later operation is a fixed sequence of fp64 + - * / sqrt, so the result is reproducible
// bit for bit (tests/consist_ref.py restates it in numpy).
#include "pf_lm.hpp"

namespace pf {

static constexpr int kLanes = 256;
static constexpr int kPairSums = 36;   // 10 of u u', 10 of v v', 16 of u v' (row-major)
static constexpr int kPairGroup = 12;  // sums reduced per LDS round: 12 x 256 doubles = 24 KB
static constexpr int kDataSums = 15;   // k_register's
// the solve keeps the matrix, b and z in LDS while they fit kSolveLds bytes
static constexpr int kSolveLds = 60 * 1024;

// Does registration sample s of tile p fall inside tile q's window?  ep / eq: the tile elements
// (k_regidx's arithmetic for p; Value()'s index at the unclamped (x, y) for q).
__device__ __forceinline__ bool pair_sample(const TileGeom& gp, const TileGeom& gq,
                                            const RegGrid& rg, const GridCol* __restrict__ rcols,
                                            const GridRow* __restrict__ rrows, int s, int& ep,
                                            int& eq)
{
    const int ncol = rg.cols + 1;
    const int r = s / ncol, c = s - r * ncol;
    const GridCol cc = rcols[rg.col_off + c];
    const GridRow rr = rrows[rg.row_off + r];
    float x, y;
    sph_to_2d(gq, rr.sz, rr.cz, cc.ca, cc.sa, x, y);
    const float den = sph_den(gq, rr.sz, rr.cz, cc.ca, cc.sa);
    if (!(den > 0.0f && x >= 0.0f && x <= 1.0f && y >= 0.0f && y <= 1.0f)) return false;
    eq = (int)tile_index(gq, x, y);
    sph_to_2d(gp, rr.sz, rr.cz, cc.ca, cc.sa, x, y);
    if (x < 0) x = 0;
    if (x > 1) x = 1;
    if (y < 0) y = 0;
    if (y > 1) y = 1;
    ep = (int)tile_index(gp, x, y);
    return true;
}

// Pass 1: block (p, q) counts |O_pq| (wave ballots, summed through LDS).
__global__ void __launch_bounds__(kLanes) k_paircount(const TileGeom* __restrict__ geom,
                                                      const RegGrid* __restrict__ grids,
                                                      const GridCol* __restrict__ rcols,
                                                      const GridRow* __restrict__ rrows,
                                                      int ntiles, int* __restrict__ counts)
{
    __shared__ int part[kLanes / 64];
    const int p = blockIdx.x / ntiles, q = blockIdx.x - p * ntiles, l = threadIdx.x;
    if (p == q) {
        if (l == 0) counts[blockIdx.x] = 0;
        return;
    }
    const TileGeom gp = geom[p], gq = geom[q];
    const RegGrid rg = grids[p];
    const int ns = (rg.cols + 1) * (rg.rows + 1);
    int n = 0;  // wave-uniform
    for (int s0 = 0; s0 < ns; s0 += kLanes) {
        const int s = s0 + l;
        int ep, eq;
        const bool keep = s < ns && pair_sample(gp, gq, rg, rcols, rrows, s, ep, eq);
        n += __popcll(__ballot(keep));
    }
    if ((l & 63) == 0) part[l >> 6] = n;
    __syncthreads();
    if (l == 0) counts[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// Pass 2: block i fills the samples of pair i = {p, q, first, count} in ascending sample order:
// per 256 samples the kept ones are numbered by ballot prefix (lanes in order, waves in order).
__global__ void __launch_bounds__(kLanes) k_pairidx(const TileGeom* __restrict__ geom,
                                                    const RegGrid* __restrict__ grids,
                                                    const GridCol* __restrict__ rcols,
                                                    const GridRow* __restrict__ rrows,
                                                    const int4* __restrict__ pairs,
                                                    int2* __restrict__ index)
{
    __shared__ int wcount[kLanes / 64];
    const int4 pr = pairs[blockIdx.x];
    const int l = threadIdx.x, wave = l >> 6, lane = l & 63;
    const TileGeom gp = geom[pr.x], gq = geom[pr.y];
    const RegGrid rg = grids[pr.x];
    const int ns = (rg.cols + 1) * (rg.rows + 1);
    int base = 0;  // block-uniform
    for (int s0 = 0; s0 < ns; s0 += kLanes) {
        const int s = s0 + l;
        int ep = 0, eq = 0;
        const bool keep = s < ns && pair_sample(gp, gq, rg, rcols, rrows, s, ep, eq);
        const unsigned long long m = __ballot(keep);
        if (lane == 0) wcount[wave] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < kLanes / 64; w++) {
            if (w < wave) before += wcount[w];
            total += wcount[w];
        }
        const int k = base + before + __popcll(m & ((1ull << lane) - 1ull));
        if (keep && k < pr.w) index[pr.z + k] = make_int2(ep, eq);  // k < count: bounds
        base += total;
        __syncthreads();
    }
}

// The halving tree of k_register on `n` sums held as part[k][lane].
template <int N>
__device__ __forceinline__ void tree_reduce(double (*part)[kLanes], int l)
{
    __syncthreads();
    for (int stride = kLanes / 2; stride >= 1; stride >>= 1) {
        if (l < stride)
            for (int k = 0; k < N; k++) part[k][l] = part[k][l] + part[k][l + stride];
        __syncthreads();
    }
}

// Pair moments: one workgroup per (panorama, pair), k_register's XCD-contiguous block order.
// out [batch][npairs][36]: U (10, k_register's order), V (10), C = sum u v' (16, row-major).
__global__ void __launch_bounds__(kLanes) k_pair_moments(
    const TileGeom* __restrict__ geom, const int4* __restrict__ pairs, int npairs,
    const int2* __restrict__ index, const float* __restrict__ tiles, long long tstride,
    double* __restrict__ out)
{
    __shared__ double part[kPairGroup][kLanes];
    const unsigned lb = xcd_remap(blockIdx.x, gridDim.x);
    const int i = (int)(lb % (unsigned)npairs), b = (int)(lb / (unsigned)npairs), l = threadIdx.x;
    const int4 pr = pairs[i];
    const float* tp = tiles + b * tstride + geom[pr.x].off;
    const float* tq = tiles + b * tstride + geom[pr.y].off;
    const int2* ix = index + pr.z;
    double acc[kPairSums];
#pragma unroll
    for (int k = 0; k < kPairSums; k++) acc[k] = 0.0;
    for (int s = l; s < pr.w; s += kLanes) {
        const int2 e = ix[s];
        const double X = clamp_sample((double)tp[e.x]);
        const double Z = clamp_sample((double)tq[e.y]);
        const double X2 = X * X, X3 = X * X * X;
        const double Z2 = Z * Z, Z3 = Z * Z * Z;
        acc[0] = acc[0] + X3 * X3; acc[1] = acc[1] + X3 * X2; acc[2] = acc[2] + X3 * X;
        acc[3] = acc[3] + X3;      acc[4] = acc[4] + X2 * X2; acc[5] = acc[5] + X2 * X;
        acc[6] = acc[6] + X2;      acc[7] = acc[7] + X * X;   acc[8] = acc[8] + X;
        acc[9] = acc[9] + 1.0;
        acc[10] = acc[10] + Z3 * Z3; acc[11] = acc[11] + Z3 * Z2; acc[12] = acc[12] + Z3 * Z;
        acc[13] = acc[13] + Z3;      acc[14] = acc[14] + Z2 * Z2; acc[15] = acc[15] + Z2 * Z;
        acc[16] = acc[16] + Z2;      acc[17] = acc[17] + Z * Z;   acc[18] = acc[18] + Z;
        acc[19] = acc[19] + 1.0;
        acc[20] = acc[20] + X3 * Z3; acc[21] = acc[21] + X3 * Z2; acc[22] = acc[22] + X3 * Z;
        acc[23] = acc[23] + X3;
        acc[24] = acc[24] + X2 * Z3; acc[25] = acc[25] + X2 * Z2; acc[26] = acc[26] + X2 * Z;
        acc[27] = acc[27] + X2;
        acc[28] = acc[28] + X * Z3;  acc[29] = acc[29] + X * Z2;  acc[30] = acc[30] + X * Z;
        acc[31] = acc[31] + X;
        acc[32] = acc[32] + Z3;      acc[33] = acc[33] + Z2;      acc[34] = acc[34] + Z;
        acc[35] = acc[35] + 1.0;
    }
    // 36 x 256 doubles exceed the LDS allocation: three rounds of 12 sums.  The tree of one sum
    // does not depend on the others, so the grouping changes no bit.
    double* o = out + ((long long)b * npairs + i) * kPairSums;
#pragma unroll
    for (int g = 0; g < kPairSums / kPairGroup; g++) {
#pragma unroll
        for (int k = 0; k < kPairGroup; k++) part[k][l] = acc[g * kPairGroup + k];
        tree_reduce<kPairGroup>(part, l);
        if (l < kPairGroup) o[g * kPairGroup + l] = part[l][0];
        __syncthreads();
    }
}

// ---- assemble and solve -----------------------------------------------------------------------
// position of (i, j) of a symmetric 4 x 4 in k_register's 10 upper products
__device__ __forceinline__ int sym10(int i, int j)
{
    const int idx[4][4] = {{0, 1, 2, 3}, {1, 4, 5, 6}, {2, 5, 7, 8}, {3, 6, 8, 9}};
    return idx[i][j];
}

// the pair (p, q) in the list sorted by (p, q); -1: none
__device__ __forceinline__ int find_pair(const int4* __restrict__ pairs, int npairs, int p, int q)
{
    int lo = 0, hi = npairs - 1;
    while (lo <= hi) {
        const int mid = (lo + hi) >> 1;
        const int4 m = pairs[mid];
        if (m.x == p && m.y == q) return mid;
        if (m.x < p || (m.x == p && m.y < q)) lo = mid + 1;
        else hi = mid - 1;
    }
    return -1;
}

// c' S d of a 4 x 4 (mom_cost's loop order): for i: t = sum_j S[i][j] d[j]; acc += c[i] t
template <class F>
__device__ __forceinline__ double quad4(F S, const double* c, const double* d)
{
    double acc = 0.0;
    for (int i = 0; i < 4; i++) {
        double t = 0.0;
        for (int j = 0; j < 4; j++) t = t + S(i, j) * d[j];
        acc = acc + c[i] * t;
    }
    return acc;
}

// One workgroup per panorama.  A (n rows of n + 1, row-major, lower triangle used), bv and zv (n each) live
// in LDS (ws == nullptr) or in the panorama's slice of the global workspace.
// summary [batch][4]: {data cost, pair cost (without the factor lambda), pair samples, status}.
__global__ void __launch_bounds__(kLanes) k_consist_solve(
    const double* __restrict__ dsums, const double* __restrict__ psums,
    const int4* __restrict__ pairs, int npairs, int ntiles, double lambda, double pair_samples,
    double* ws, float* __restrict__ coeffs, double* __restrict__ coeffs64,
    double* __restrict__ summary)
{
    extern __shared__ double lds[];
    const int b = blockIdx.x, l = threadIdx.x, n = 4 * ntiles;
    // rows are ld = n + 1 doubles apart: n is a multiple of 4, and a column walk (L_jk over j) at an
    // even stride would land on two LDS banks; the odd stride spreads it over all of them
    const int ld = n + 1;
    const long long nn = (long long)ld * n;
    double* A = ws ? ws + (long long)b * (nn + 2 * n) : lds;
    double* bv = A + nn;
    double* zv = bv + n;
    const double* D = dsums + (long long)b * ntiles * kDataSums;
    const double* P = psums + (long long)b * npairs * kPairSums;

    for (long long e = l; e < nn; e += kLanes) A[e] = 0.0;
    __syncthreads();
    // diagonal blocks: M_p, then lambda U_pq in ascending q, then lambda V_qp in ascending q
    for (int p = l; p < ntiles; p += kLanes) {
        double blk[10];
        for (int k = 0; k < 10; k++) blk[k] = D[p * kDataSums + k];
        for (int i = 0; i < npairs; i++)
            if (pairs[i].x == p)
                for (int k = 0; k < 10; k++) blk[k] = blk[k] + lambda * P[i * kPairSums + k];
        for (int i = 0; i < npairs; i++)
            if (pairs[i].y == p)
                for (int k = 0; k < 10; k++) blk[k] = blk[k] + lambda * P[i * kPairSums + 10 + k];
        for (int i = 0; i < 4; i++) {
            for (int j = 0; j <= i; j++) A[(long long)(4 * p + i) * ld + 4 * p + j] = blk[sym10(i, j)];
            bv[4 * p + i] = D[p * kDataSums + 10 + i];
        }
    }
    // off-diagonal blocks (a > b): A_ab = -(lambda (C_ab + C_ba')), a missing pair counting as 0.0
    for (int i = l; i < npairs; i += kLanes) {
        const int p = pairs[i].x, q = pairs[i].y;
        const int rev = find_pair(pairs, npairs, q, p);
        int ia, ib, a, bb;  // pair (a, b) and pair (b, a), a > b
        if (p > q) { a = p; bb = q; ia = i; ib = rev; }
        else if (rev < 0) { a = q; bb = p; ia = -1; ib = i; }
        else continue;  // the reverse pair's lane writes the block
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) {
                const double cab = ia >= 0 ? P[ia * kPairSums + 20 + r * 4 + c] : 0.0;
                const double cba = ib >= 0 ? P[ib * kPairSums + 20 + c * 4 + r] : 0.0;
                A[(long long)(4 * a + r) * ld + 4 * bb + c] = -(lambda * (cab + cba));
            }
    }
    __syncthreads();

    // Cholesky, right-looking, in place.  Every element sees its updates in ascending k.
    bool bad = false;  // block-uniform: every lane reads the same pivot
    for (int k = 0; k < n; k++) {
        const double akk = A[(long long)k * ld + k];
        if (!(akk > 0.0)) { bad = true; break; }
        const double d = sqrt(akk);
        __syncthreads();  // every lane has read A_kk
        if (l == 0) A[(long long)k * ld + k] = d;
        for (int i = k + 1 + l; i < n; i += kLanes)
            A[(long long)i * ld + k] = A[(long long)i * ld + k] / d;
        __syncthreads();
        const int m = n - k - 1;
        for (int e = l; e < m * m; e += kLanes) {
            const int i = k + 1 + e / m, j = k + 1 + e % m;
            if (j <= i)
                A[(long long)i * ld + j] =
                    A[(long long)i * ld + j] - A[(long long)i * ld + k] * A[(long long)j * ld + k];
        }
        __syncthreads();
    }
    if (!bad) {
        // forward: z_k = b_k / L_kk, b_i = b_i - L_ik z_k (i > k)
        for (int k = 0; k < n; k++) {
            const double zk = bv[k] / A[(long long)k * ld + k];
            if (l == 0) zv[k] = zk;
            for (int i = k + 1 + l; i < n; i += kLanes) bv[i] = bv[i] - A[(long long)i * ld + k] * zk;
            __syncthreads();
        }
        // backward: c_k = z_k / L_kk, z_i = z_i - L_ki c_k (i < k); c goes to bv
        for (int k = n - 1; k >= 0; k--) {
            const double ck = zv[k] / A[(long long)k * ld + k];
            if (l == 0) bv[k] = ck;
            for (int i = l; i < k; i += kLanes) zv[i] = zv[i] - A[(long long)k * ld + i] * ck;
            __syncthreads();
        }
        for (int i = 0; i < n; i++) bad = bad || !isfinite(bv[i]);  // block-uniform
    }
    if (bad) {
        for (int i = l; i < n; i += kLanes) {
            if (coeffs) coeffs[(long long)b * n + i] = __uint_as_float(0x7FC00000u);
            if (coeffs64) coeffs64[(long long)b * n + i] = __longlong_as_double(0x7FF8000000000000LL);
        }
        if (l == 0 && summary) {
            summary[b * 4 + 0] = __longlong_as_double(0x7FF8000000000000LL);
            summary[b * 4 + 1] = __longlong_as_double(0x7FF8000000000000LL);
            summary[b * 4 + 2] = pair_samples;
            summary[b * 4 + 3] = 1.0;
        }
        return;
    }
    for (int i = l; i < n; i += kLanes) {
        if (coeffs) coeffs[(long long)b * n + i] = (float)bv[i];
        if (coeffs64) coeffs64[(long long)b * n + i] = bv[i];
    }
    if (!summary) return;
    // the two terms of E from the moment sums; the factor is done with, A holds the terms:
    // A[p] = (yy - 2 c'J'y) + c'M c of tile p, A[ntiles + i] = (c'U c - 2 c'C d) + d'V d of pair i
    __syncthreads();
    for (int p = l; p < ntiles; p += kLanes) {
        const double* S = D + p * kDataSums;
        const double* c = bv + 4 * p;
        const double cMc = quad4([&](int i, int j) { return S[sym10(i, j)]; }, c, c);
        double cJy = 0.0;
        for (int i = 0; i < 4; i++) cJy = cJy + c[i] * S[10 + i];
        A[p] = (S[14] - 2.0 * cJy) + cMc;
    }
    for (int i = l; i < npairs; i += kLanes) {
        const double* S = P + i * kPairSums;
        const double* c = bv + 4 * pairs[i].x;
        const double* d = bv + 4 * pairs[i].y;
        const double cUc = quad4([&](int r, int k) { return S[sym10(r, k)]; }, c, c);
        const double dVd = quad4([&](int r, int k) { return S[10 + sym10(r, k)]; }, d, d);
        const double cCd = quad4([&](int r, int k) { return S[20 + r * 4 + k]; }, c, d);
        A[ntiles + i] = (cUc - 2.0 * cCd) + dVd;
    }
    __syncthreads();
    if (l == 0) {
        double dc = 0.0, pc = 0.0;
        for (int p = 0; p < ntiles; p++) dc = dc + A[p];
        for (int i = 0; i < npairs; i++) pc = pc + A[ntiles + i];
        summary[b * 4 + 0] = dc;
        summary[b * 4 + 1] = pc;
        summary[b * 4 + 2] = pair_samples;
        summary[b * 4 + 3] = 0.0;
    }
}

// Overlap statistics: one workgroup per (panorama, pair), the lane order and tree of the moments.
// d = (double)T32_p - (double)T32_q, T32 = cubic_map's value (coeffs == nullptr: the raw values).
// out [batch][npairs][5] = {count, sum d, sum d^2, max |d|, samples with a NaN on either side}.
__global__ void __launch_bounds__(kLanes) k_overlap_stats(
    const TileGeom* __restrict__ geom, const int4* __restrict__ pairs, int npairs, int ntiles,
    const int2* __restrict__ index, const float* __restrict__ tiles, long long tstride,
    const float* __restrict__ coeffs, double* __restrict__ out)
{
    __shared__ double part[5][kLanes];
    const unsigned lb = xcd_remap(blockIdx.x, gridDim.x);
    const int i = (int)(lb % (unsigned)npairs), b = (int)(lb / (unsigned)npairs), l = threadIdx.x;
    const int4 pr = pairs[i];
    const float* tp = tiles + b * tstride + geom[pr.x].off;
    const float* tq = tiles + b * tstride + geom[pr.y].off;
    const int2* ix = index + pr.z;
    float cp[4] = {0, 0, 0, 0}, cq[4] = {0, 0, 0, 0};
    if (coeffs)
        for (int k = 0; k < 4; k++) {
            cp[k] = coeffs[((long long)b * ntiles + pr.x) * 4 + k];
            cq[k] = coeffs[((long long)b * ntiles + pr.y) * 4 + k];
        }
    double cnt = 0.0, sd = 0.0, sdd = 0.0, mx = 0.0, nans = 0.0;
    for (int s = l; s < pr.w; s += kLanes) {
        const int2 e = ix[s];
        float vp = tp[e.x], vq = tq[e.y];
        if (coeffs) {
            vp = cubic_map(vp, cp[0], cp[1], cp[2], cp[3]);
            vq = cubic_map(vq, cq[0], cq[1], cq[2], cq[3]);
        }
        if (vp != vp || vq != vq) {
            nans = nans + 1.0;
            continue;
        }
        const double d = (double)vp - (double)vq;
        cnt = cnt + 1.0;
        sd = sd + d;
        sdd = sdd + d * d;
        const double ad = fabs(d);
        if (ad > mx) mx = ad;
    }
    part[0][l] = cnt; part[1][l] = sd; part[2][l] = sdd; part[3][l] = mx; part[4][l] = nans;
    __syncthreads();
    for (int stride = kLanes / 2; stride >= 1; stride >>= 1) {
        if (l < stride) {
            part[0][l] = part[0][l] + part[0][l + stride];
            part[1][l] = part[1][l] + part[1][l + stride];
            part[2][l] = part[2][l] + part[2][l + stride];
            if (part[3][l + stride] > part[3][l]) part[3][l] = part[3][l + stride];
            part[4][l] = part[4][l] + part[4][l + stride];
        }
        __syncthreads();
    }
    if (l < 5) out[((long long)b * npairs + i) * 5 + l] = part[l][0];
}

// ---- launchers --------------------------------------------------------------------------------
void launch_paircount(hipStream_t s, const TileGeom* geom, const RegGrid* grids,
                      const GridCol* rcols, const GridRow* rrows, int ntiles, int* counts)
{
    hipLaunchKernelGGL(k_paircount, dim3((unsigned)(ntiles * ntiles)), dim3(kLanes), 0, s, geom,
                       grids, rcols, rrows, ntiles, counts);
}

void launch_pairidx(hipStream_t s, const TileGeom* geom, const RegGrid* grids,
                    const GridCol* rcols, const GridRow* rrows, const int* pairs, int npairs,
                    int2* index)
{
    hipLaunchKernelGGL(k_pairidx, dim3((unsigned)npairs), dim3(kLanes), 0, s, geom, grids, rcols,
                       rrows, (const int4*)pairs, index);
}

int pair_sums_per_pair() { return kPairSums; }

void launch_pair_moments(hipStream_t s, const TileGeom* geom, const int* pairs, int npairs,
                         const int2* index, const float* tiles, long long tstride, double* out,
                         int batch)
{
    hipLaunchKernelGGL(k_pair_moments, dim3((unsigned)(npairs * batch)), dim3(kLanes), 0, s, geom,
                       (const int4*)pairs, npairs, index, tiles, tstride, out);
}

bool consist_fits_lds(int ntiles)
{
    return consist_workspace_doubles(ntiles) * sizeof(double) <= (size_t)kSolveLds;
}

size_t consist_workspace_doubles(int ntiles)
{
    const size_t n = 4 * (size_t)ntiles;
    return (n + 1) * n + 2 * n;  // the matrix at a row stride of n + 1, then b and z
}

void launch_consist_solve(hipStream_t s, const double* dsums, const double* psums,
                          const int* pairs, int npairs, int ntiles, double lambda,
                          double pair_samples, double* ws, float* coeffs, double* coeffs64,
                          double* summary, int batch)
{
    const size_t lds = ws ? 0 : consist_workspace_doubles(ntiles) * sizeof(double);
    hipLaunchKernelGGL(k_consist_solve, dim3((unsigned)batch), dim3(kLanes), lds, s, dsums, psums,
                       (const int4*)pairs, npairs, ntiles, lambda, pair_samples, ws, coeffs,
                       coeffs64, summary);
}

void launch_overlap_stats(hipStream_t s, const TileGeom* geom, const int* pairs, int npairs,
                          int ntiles, const int2* index, const float* tiles, long long tstride,
                          const float* coeffs, double* out, int batch)
{
    hipLaunchKernelGGL(k_overlap_stats, dim3((unsigned)(npairs * batch)), dim3(kLanes), 0, s,
                       geom, (const int4*)pairs, npairs, ntiles, index, tiles, tstride, coeffs,
                       out);
}

}  // namespace pf
