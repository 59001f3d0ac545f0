// pf_register.hip -- the moment-form cubic registration: the 15 fp64 moment sums of a tile's samples
// (k_register, k_register_valid; k_register_weighted with a weight per sample), their solve by least squares or by the reference's Ceres 1.13
// trust-region LM (lm_moments over lm_solve, pf_lm.hpp), the joint and global solves on the same
// sums (k_register_joint, k_global_solve), the cached sample indices (k_regidx) and
// Depth2DepthTransform (k_apply_cubic, k_d2d_map); for planar-depth tiles (pf_set_tile_depth) the
// ray factor (k_ray_factor, k_reg_kf), the moment sums weighted by it (k_register_planar,
// k_register_planar_valid) and the transform composed with it (k_apply_cubic_planar).
#include "pf_lm.hpp"

namespace pf {

static constexpr int kBlock = 256;
static inline unsigned nblocks(long long n) { return (unsigned)((n + kBlock - 1) / kBlock); }

// ---------------------------------------------------------------------------------------------
// Registration: one workgroup per (tile, panorama).  Lane l accumulates the 15 fp64 sums of
// J^T J / J^T y / y^T y over samples l, l+256, ... (J = (x^3, x^2, x, 1) of FunctorDepth2Depth3,
// Depth.cpp:1122-1138), then a fixed pairwise tree; lane 0 solves.  The order is fixed, so the
// result is reproducible and identical to the oracle's restatement.
static constexpr int kRegLanes = 256;
static constexpr int kRegSums = 15;

__device__ int solve_normal(const double* S, int degree, double* coef)
{
    const int idx[4][4] = {{0, 1, 2, 3}, {1, 4, 5, 6}, {2, 5, 7, 8}, {3, 6, 8, 9}};
    int n = degree + 1, off = 3 - degree;
    double A[4][5];
    for (int i = 0; i < n; i++) {
        for (int j = 0; j < n; j++) A[i][j] = S[idx[i + off][j + off]];
        A[i][n] = S[10 + i + off];
    }
    for (int k = 0; k < n; k++) {
        int piv = k;
        double best = fabs(A[k][k]);
        for (int i = k + 1; i < n; i++)
            if (fabs(A[i][k]) > best) { best = fabs(A[i][k]); piv = i; }
        if (!(best > 0.0)) return -1;
        if (piv != k)
            for (int j = 0; j <= n; j++) { double t = A[k][j]; A[k][j] = A[piv][j]; A[piv][j] = t; }
        for (int i = k + 1; i < n; i++) {
            double f = A[i][k] / A[k][k];
            for (int j = k; j <= n; j++) A[i][j] = A[i][j] - f * A[k][j];
        }
    }
    for (int i = n - 1; i >= 0; i--) {
        double s = A[i][n];
        for (int j = i + 1; j < n; j++) s = s - A[i][j] * coef[j];
        coef[i] = s / A[i][i];
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------
// The reference's registration solver (lm_solve, pf_lm.hpp) from `start` ((1,1,1,1) for
// SolveDepthToDepth, Depth.cpp:1270-1274, 1399-1404; (0,0,1,0) for SolveDepthToDepth2,
// Depth.cpp:1169-1173), evaluated from the 15 moment sums -- the residuals are linear in
// (a,b,c,d), so cost, gradient and J'J are exact functions of them.  pfo_lm_moments
// (oracle/pf_oracle_lm.c) is this function operation for operation (fp64 +, -, *, /, sqrt only,
// no contraction), so the two agree bit for bit.  summary (optional): {initial cost, final cost,
// iterations, termination} in pf_register_disparity's encoding.
namespace {
struct Mom {
    double M[4][4], Jy[4], yy;
};

__device__ double mom_cost(const Mom& m, const double p[4])
{
    double pMp = 0.0, pJy = 0.0;
    for (int i = 0; i < 4; i++) {
        double q = 0.0;
        for (int j = 0; j < 4; j++) q = q + m.M[i][j] * p[j];
        pMp = pMp + p[i] * q;
        pJy = pJy + p[i] * m.Jy[i];
    }
    return 0.5 * ((m.yy - 2.0 * pJy) + pMp);
}

__device__ void mom_gradient(const Mom& m, const double p[4], double g[4])
{
    for (int i = 0; i < 4; i++) {
        double q = 0.0;
        for (int j = 0; j < 4; j++) q = q + m.M[i][j] * p[j];
        g[i] = q - m.Jy[i];
    }
}
}  // namespace

__device__ void lm_moments(const double* S, const double (&start)[4], double (&coef)[4],
                           double* summary = nullptr)
{
    Mom m;
    const int idx[4][4] = {{0, 1, 2, 3}, {1, 4, 5, 6}, {2, 5, 7, 8}, {3, 6, 8, 9}};
    for (int i = 0; i < 4; i++) {
        for (int j = 0; j < 4; j++) m.M[i][j] = S[idx[i][j]];
        m.Jy[i] = S[10 + i];
    }
    m.yy = S[14];
    LmSummary sm;
    lm_solve<4, false>(
        start,
        [&](const double (&x)[4], double& cost, double (&g)[4], double (&M)[4][4]) {
            cost = mom_cost(m, x);
            mom_gradient(m, x, g);
            for (int i = 0; i < 4; i++)
                for (int j = 0; j < 4; j++) M[i][j] = m.M[i][j];
        },
        [&](const double (&x)[4]) { return mom_cost(m, x); }, coef, sm);
    if (summary) {
        summary[0] = sm.initial_cost;
        summary[1] = sm.final_cost;
        summary[2] = (double)sm.iterations;
        summary[3] = (double)sm.termination;
    }
}

// Degree-d least squares from the normal-equation sums (falling back to lower degrees when the
// system is singular), stored as {a, b, c, d} with the unused high-order terms 0.
__device__ void solve_store(const double* S, int degree, int solver, float* coeffs,
                            double* coeffs64, long long o)
{
    if (solver == PF_SOLVER_LM && degree == 3) {
        const double ones[4] = {1.0, 1.0, 1.0, 1.0};
        double c[4];
        lm_moments(S, ones, c);
        for (int i = 0; i < 4; i++) {
            if (coeffs) coeffs[o + i] = (float)c[i];  // Vec4f(vars), Depth.cpp:1408
            if (coeffs64) coeffs64[o + i] = c[i];
        }
        return;
    }
    double coef[4] = {0, 0, 0, 0};
    int d = degree, rc = -1;
    while (d >= 0 && (rc = solve_normal(S, d, coef)) != 0) d--;
    if (rc != 0) { coef[0] = 0.0; d = 0; }
    double full[4] = {0, 0, 0, 0};
    for (int i = 0; i <= d; i++) full[3 - d + i] = coef[i];
    for (int i = 0; i < 4; i++) {
        if (coeffs) coeffs[o + i] = (float)full[i];
        if (coeffs64) coeffs64[o + i] = full[i];
    }
}

// The masked rule's store (pf_set_tile_validity): four quiet NaNs for a problem with fewer than
// degree + 1 valid samples (count: S[9] for the plain sums, the 16th sum under the ray factor,
// whose S[9] is the sum of K K) or with a non-finite solution.
__device__ void solve_store_valid(const double* S, int degree, int solver, float* coeffs,
                                  double* coeffs64, long long o, double count)
{
    float c32[4];
    double c64[4];
    bool ok = count >= (double)(degree + 1);
    if (ok) {
        solve_store(S, degree, solver, c32, c64, 0);
        for (int i = 0; i < 4; i++) ok = ok && isfinite(c64[i]);
    }
    for (int i = 0; i < 4; i++) {
        if (coeffs) coeffs[o + i] = ok ? c32[i] : __uint_as_float(0x7FC00000u);
        if (coeffs64) coeffs64[o + i] = ok ? c64[i] : __longlong_as_double(0x7FF8000000000000LL);
    }
}

__device__ void solve_store_valid(const double* S, int degree, int solver, float* coeffs,
                                  double* coeffs64, long long o)
{
    solve_store_valid(S, degree, solver, coeffs, coeffs64, o, S[9]);
}

// One block's registration of tile p of panorama b.  MASK (k_register_valid): a sample whose raw
// tile value fails the rule, or whose baseline value is not finite, adds nothing to the sums; the
// lane-to-sample assignment and the halving tree are the unmasked ones, so acc[9] is the count of
// valid samples.  With MASK false this is k_register as it was.
// PLANAR (k_register_planar, k_register_planar_valid; pf_set_tile_depth): the tile holds depth along
// the optical axis, so the model is K (a X^3 + b X^2 + c X + d) with K = (double)kfs[sample], the
// sample's ray factor (k_reg_kf).  The Jacobian row is e = (K X^3, K X^2, K X, K) and the 15 sums
// keep their positions with e in place of (X^3, X^2, X, 1): they are J'J, J'y and y'y of the
// weighted problem, which solve_normal and lm_moments take unchanged.  acc[9] is then the sum of
// K K, so under MASK the count of valid samples travels in a 16th sum.  Needs sidx.
template <bool MASK, bool PLANAR = false>
__device__ __forceinline__ void register_tile(
    const TileGeom* __restrict__ geom, const RegGrid* __restrict__ grids,
    const GridCol* __restrict__ rcols, const GridRow* __restrict__ rrows, int ntiles,
    const float* __restrict__ emap, int ew, int eh, int ec, long long estride,
    const float* __restrict__ tiles, long long tstride, int degree, int solver,
    float* __restrict__ coeffs, double* __restrict__ coeffs64, double* __restrict__ sums,
    const int* __restrict__ active, const int2* __restrict__ sidx, float vlo, float vhi,
    double (*part)[kRegLanes], const float* __restrict__ kfs = nullptr)
{
    constexpr int kNS = PLANAR && MASK ? kRegSums + 1 : kRegSums;
    // one linear grid, XCD-contiguous: the tiles of one panorama run on one XCD, so its emap is
    // fetched into one L2 (the samples of neighbouring tiles overlap in the emap)
    const unsigned lb = xcd_remap(blockIdx.x, gridDim.x);
    const int p = (int)(lb % (unsigned)ntiles), b = (int)(lb / (unsigned)ntiles), l = threadIdx.x;
    if (active && !active[p]) return;  // joint solve: an inactive tile is neither read nor solved
    const TileGeom g = geom[p];
    const RegGrid rg = grids[p];
    const float* tile = tiles + b * tstride + g.off;
    const float* em = emap + b * estride;
    const int ncol = rg.cols + 1;
    const int ns = ncol * (rg.rows + 1);
    double acc[kNS];
#pragma unroll
    for (int k = 0; k < kNS; k++) acc[k] = 0.0;
    // The lane's samples l, l + 256, ... in groups of kRegU: the gathers of a group are issued
    // together (they are independent), then added in sample order -- the same per-lane order as
    // one sample per iteration, so the sums are unchanged bit for bit.
    constexpr int kRegU = 4;
    for (int s0 = l; s0 < ns; s0 += kRegU * kRegLanes) {
        float tv[kRegU], ev[kRegU];
        float kv[PLANAR ? kRegU : 1];
#pragma unroll
        for (int u = 0; u < kRegU; u++) {
            const int s = s0 + u * kRegLanes;
            tv[u] = 0.0f;
            ev[u] = 0.0f;
            if constexpr (PLANAR) kv[u] = 1.0f;
            if (s >= ns) continue;
            if (PLANAR || sidx) {  // the cached indices (k_regidx: the same arithmetic as below)
                const int2 ix = sidx[rg.soff + s];
                tv[u] = tile[ix.x];
                ev[u] = em[ix.y];
                if constexpr (PLANAR) kv[u] = kfs[rg.soff + s];
                continue;
            }
            int r = s / ncol, c = s - r * ncol;
            const GridCol cc = rcols[rg.col_off + c];
            const GridRow rr = rrows[rg.row_off + r];
            float x, y;
            sph_to_2d(g, rr.sz, rr.cz, cc.ca, cc.sa, x, y);
            if (x < 0) x = 0;
            if (x > 1) x = 1;
            if (y < 0) y = 0;
            if (y > 1) y = 1;
            tv[u] = tile[tile_index(g, x, y)];
            ev[u] = em[emap_index(cc.az, rr.zen, ew, eh, ec)];
        }
#pragma unroll
        for (int u = 0; u < kRegU; u++) {
            if (s0 + u * kRegLanes >= ns) break;
            if constexpr (MASK)
                if (!(tile_ok(tv[u], vlo, vhi) && isfinite(ev[u]))) continue;
            double X = clamp_sample((double)tv[u]);
            double Yv = clamp_sample((double)ev[u]);
            double X2 = X * X, X3 = X * X * X;
            if constexpr (PLANAR) {
                const double K = (double)kv[u];
                const double e3 = K * X3, e2 = K * X2, e1 = K * X, e0 = K;
                acc[0] = acc[0] + e3 * e3; acc[1] = acc[1] + e3 * e2; acc[2] = acc[2] + e3 * e1;
                acc[3] = acc[3] + e3 * e0; acc[4] = acc[4] + e2 * e2; acc[5] = acc[5] + e2 * e1;
                acc[6] = acc[6] + e2 * e0; acc[7] = acc[7] + e1 * e1; acc[8] = acc[8] + e1 * e0;
                acc[9] = acc[9] + e0 * e0;
                acc[10] = acc[10] + e3 * Yv; acc[11] = acc[11] + e2 * Yv;
                acc[12] = acc[12] + e1 * Yv; acc[13] = acc[13] + e0 * Yv;
                acc[14] = acc[14] + Yv * Yv;
                if constexpr (MASK) acc[15] = acc[15] + 1.0;
                continue;
            }
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
    for (int k = 0; k < kNS; k++) part[k][l] = acc[k];
    __syncthreads();
    for (int stride = kRegLanes / 2; stride >= 1; stride >>= 1) {
        if (l < stride)
            for (int k = 0; k < kNS; k++) part[k][l] = part[k][l] + part[k][l + stride];
        __syncthreads();
    }
    if (l == 0) {
        double S[kNS];
        for (int k = 0; k < kNS; k++) S[k] = part[k][0];
        if (sums) {  // joint solve: hand the tile's normal-equation sums to k_register_joint
            for (int k = 0; k < kRegSums; k++) sums[((long long)b * ntiles + p) * kRegSums + k] = S[k];
            return;
        }
        if constexpr (MASK && PLANAR)
            solve_store_valid(S, degree, solver, coeffs, coeffs64, ((long long)b * ntiles + p) * 4,
                              S[kRegSums]);
        else if constexpr (MASK)
            solve_store_valid(S, degree, solver, coeffs, coeffs64, ((long long)b * ntiles + p) * 4);
        else
            solve_store(S, degree, solver, coeffs, coeffs64, ((long long)b * ntiles + p) * 4);
    }
}

__global__ void __launch_bounds__(kRegLanes) k_register(
    const TileGeom* __restrict__ geom, const RegGrid* __restrict__ grids,
    const GridCol* __restrict__ rcols, const GridRow* __restrict__ rrows, int ntiles,
    const float* __restrict__ emap, int ew, int eh, int ec, long long estride,
    const float* __restrict__ tiles, long long tstride, int degree, int solver,
    float* __restrict__ coeffs, double* __restrict__ coeffs64, double* __restrict__ sums,
    const int* __restrict__ active, const int2* __restrict__ sidx)
{
    __shared__ double part[kRegSums][kRegLanes];
    register_tile<false>(geom, grids, rcols, rrows, ntiles, emap, ew, eh, ec, estride, tiles,
                         tstride, degree, solver, coeffs, coeffs64, sums, active, sidx, 0.0f, 0.0f,
                         part);
}

__global__ void __launch_bounds__(kRegLanes) k_register_valid(
    const TileGeom* __restrict__ geom, const RegGrid* __restrict__ grids,
    const GridCol* __restrict__ rcols, const GridRow* __restrict__ rrows, int ntiles,
    const float* __restrict__ emap, int ew, int eh, int ec, long long estride,
    const float* __restrict__ tiles, long long tstride, int degree, int solver,
    float* __restrict__ coeffs, double* __restrict__ coeffs64, double* __restrict__ sums,
    const int* __restrict__ active, const int2* __restrict__ sidx, float vlo, float vhi)
{
    __shared__ double part[kRegSums][kRegLanes];
    register_tile<true>(geom, grids, rcols, rrows, ntiles, emap, ew, eh, ec, estride, tiles,
                        tstride, degree, solver, coeffs, coeffs64, sums, active, sidx, vlo, vhi,
                        part);
}

// The same under PF_TILE_DEPTH_PLANAR: kfs is the samples' ray factor (k_reg_kf), sidx is required.
__global__ void __launch_bounds__(kRegLanes) k_register_planar(
    const TileGeom* __restrict__ geom, const RegGrid* __restrict__ grids, int ntiles,
    const float* __restrict__ emap, long long estride, const float* __restrict__ tiles,
    long long tstride, int degree, int solver, float* __restrict__ coeffs,
    double* __restrict__ coeffs64, const int2* __restrict__ sidx, const float* __restrict__ kfs)
{
    __shared__ double part[kRegSums][kRegLanes];
    register_tile<false, true>(geom, grids, nullptr, nullptr, ntiles, emap, 0, 0, 0, estride,
                               tiles, tstride, degree, solver, coeffs, coeffs64, nullptr, nullptr,
                               sidx, 0.0f, 0.0f, part, kfs);
}

__global__ void __launch_bounds__(kRegLanes) k_register_planar_valid(
    const TileGeom* __restrict__ geom, const RegGrid* __restrict__ grids, int ntiles,
    const float* __restrict__ emap, long long estride, const float* __restrict__ tiles,
    long long tstride, int degree, int solver, float* __restrict__ coeffs,
    double* __restrict__ coeffs64, const int2* __restrict__ sidx, const float* __restrict__ kfs,
    float vlo, float vhi)
{
    __shared__ double part[kRegSums + 1][kRegLanes];
    register_tile<true, true>(geom, grids, nullptr, nullptr, ntiles, emap, 0, 0, 0, estride, tiles,
                              tstride, degree, solver, coeffs, coeffs64, nullptr, nullptr, sidx,
                              vlo, vhi, part, kfs);
}

// The third form of register_tile (k_register_weighted, pf_register_weighted): per-pixel weights
// in the tiles' element layout.  Sample s of tile p is used iff its weight w = weights[sidx[s].x]
// is usable (0 < w < +inf), its raw tile value is finite and its baseline value is finite; a used
// sample adds W * t_k to sum k, W = (double)w and t_k the term k_register forms, so acc[9] is the
// sum of w and the count of used samples travels in a 16th sum.  These are J'J, J'y and y'y of
// the residuals times sqrt(w): the reference's Weight = sqrt(w) in FunctorDepth2Depth3
// (Depth.cpp:1122-1138).  The lane-to-sample order and the halving tree are k_register's, so with
// every weight 1.0f the sums are k_register's bit for bit (1.0 * t is t).  Degree 3, the LM.
__global__ void __launch_bounds__(kRegLanes) k_register_weighted(
    const TileGeom* __restrict__ geom, const RegGrid* __restrict__ grids, int ntiles,
    const float* __restrict__ emap, long long estride, const float* __restrict__ tiles,
    long long tstride, const float* __restrict__ weights, long long wstride,
    float* __restrict__ coeffs, double* __restrict__ coeffs64, double* __restrict__ summary,
    const int2* __restrict__ sidx)
{
    constexpr int kNS = kRegSums + 1;
    __shared__ double part[kNS][kRegLanes];
    const unsigned lb = xcd_remap(blockIdx.x, gridDim.x);
    const int p = (int)(lb % (unsigned)ntiles), b = (int)(lb / (unsigned)ntiles), l = threadIdx.x;
    const TileGeom g = geom[p];
    const RegGrid rg = grids[p];
    const float* tile = tiles + b * tstride + g.off;
    const float* wt = weights + b * wstride + g.off;
    const float* em = emap + b * estride;
    const int ns = (rg.cols + 1) * (rg.rows + 1);
    double acc[kNS];
#pragma unroll
    for (int k = 0; k < kNS; k++) acc[k] = 0.0;
    constexpr int kRegU = 4;  // the gathers of a group issue together, then add in sample order
    for (int s0 = l; s0 < ns; s0 += kRegU * kRegLanes) {
        float tv[kRegU], ev[kRegU], wv[kRegU];
#pragma unroll
        for (int u = 0; u < kRegU; u++) {
            const int s = s0 + u * kRegLanes;
            tv[u] = ev[u] = wv[u] = 0.0f;
            if (s >= ns) continue;
            const int2 ix = sidx[rg.soff + s];
            tv[u] = tile[ix.x];
            wv[u] = wt[ix.x];
            ev[u] = em[ix.y];
        }
#pragma unroll
        for (int u = 0; u < kRegU; u++) {
            if (s0 + u * kRegLanes >= ns) break;
            if (!(0.0f < wv[u] && wv[u] < __uint_as_float(0x7F800000u) && isfinite(tv[u]) &&
                  isfinite(ev[u])))
                continue;
            const double W = (double)wv[u];
            double X = clamp_sample((double)tv[u]);
            double Yv = clamp_sample((double)ev[u]);
            double X2 = X * X, X3 = X * X * X;
            acc[0] = acc[0] + W * (X3 * X3); acc[1] = acc[1] + W * (X3 * X2);
            acc[2] = acc[2] + W * (X3 * X);  acc[3] = acc[3] + W * X3;
            acc[4] = acc[4] + W * (X2 * X2); acc[5] = acc[5] + W * (X2 * X);
            acc[6] = acc[6] + W * X2;        acc[7] = acc[7] + W * (X * X);
            acc[8] = acc[8] + W * X;         acc[9] = acc[9] + W * 1.0;
            acc[10] = acc[10] + W * (X3 * Yv); acc[11] = acc[11] + W * (X2 * Yv);
            acc[12] = acc[12] + W * (X * Yv);  acc[13] = acc[13] + W * Yv;
            acc[14] = acc[14] + W * (Yv * Yv);
            acc[15] = acc[15] + 1.0;
        }
    }
#pragma unroll
    for (int k = 0; k < kNS; k++) part[k][l] = acc[k];
    __syncthreads();
    for (int stride = kRegLanes / 2; stride >= 1; stride >>= 1) {
        if (l < stride)
            for (int k = 0; k < kNS; k++) part[k][l] = part[k][l] + part[k][l + stride];
        __syncthreads();
    }
    if (l == 0) {
        double S[kNS];
        for (int k = 0; k < kNS; k++) S[k] = part[k][0];
        const long long o = (long long)b * ntiles + p;
        solve_store_valid(S, 3, PF_SOLVER_LM, coeffs, coeffs64, o * 4, S[kRegSums]);
        if (summary) {
            summary[o * 2] = S[kRegSums];
            summary[o * 2 + 1] = S[9];
        }
    }
}

// pf_tile_valid_counts: block (p, b) counts the registration samples k_register_valid keeps and
// the tile's pixels that pass the rule (every one with the rule off), as wave ballots summed
// through LDS.
__global__ void __launch_bounds__(256) k_valid_counts(
    const TileGeom* __restrict__ geom, const RegGrid* __restrict__ grids, int ntiles,
    const float* __restrict__ emap, long long estride, const float* __restrict__ tiles,
    long long tstride, const int2* __restrict__ sidx, TileValid tv, long long* __restrict__ counts)
{
    __shared__ long long part[4][2];
    const int p = blockIdx.x % ntiles, b = blockIdx.x / ntiles, l = threadIdx.x;
    const TileGeom g = geom[p];
    const RegGrid rg = grids[p];
    const float* tile = tiles + b * tstride + g.off;
    const float* em = emap + b * estride;
    const int ns = (rg.cols + 1) * (rg.rows + 1);
    const int npx = g.w * g.h;
    long long nsamp = 0, npix = 0;  // wave-uniform
    for (int s0 = 0; s0 < ns; s0 += 256) {
        const int s = s0 + l;
        bool ok = s < ns;
        if (ok && tv.on) {
            const int2 ix = sidx[rg.soff + s];
            ok = tile_ok(tile[ix.x], tv.lo, tv.hi) && isfinite(em[ix.y]);
        }
        nsamp += __popcll(__ballot(ok));
    }
    for (int i0 = 0; i0 < npx; i0 += 256) {
        const int i = i0 + l;
        bool ok = i < npx;
        if (ok && tv.on) ok = tile_ok(tile[(long long)i * g.c], tv.lo, tv.hi);
        npix += __popcll(__ballot(ok));
    }
    if ((l & 63) == 0) {
        part[l >> 6][0] = nsamp;
        part[l >> 6][1] = npix;
    }
    __syncthreads();
    if (l < 2)
        counts[((long long)b * ntiles + p) * 2 + l] =
            part[0][l] + part[1][l] + part[2][l] + part[3][l];
}

// SolveDepthToDepth with several active maps (Depth.cpp:1274-1376: every active map's sample
// grid feeds one problem): the active tiles' sums added in tile order, one solve per panorama.
__global__ void k_register_joint(const double* __restrict__ sums, const int* __restrict__ active,
                                 int ntiles, int batch, int degree, int solver,
                                 float* __restrict__ coeffs, double* __restrict__ coeffs64,
                                 int guard)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    double S[kRegSums];
    for (int k = 0; k < kRegSums; k++) S[k] = 0.0;
    for (int p = 0; p < ntiles; p++)
        if (active[p])
            for (int k = 0; k < kRegSums; k++)
                S[k] = S[k] + sums[((long long)b * ntiles + p) * kRegSums + k];
    if (guard) solve_store_valid(S, degree, solver, coeffs, coeffs64, (long long)b * 4);
    else solve_store(S, degree, solver, coeffs, coeffs64, (long long)b * 4);
}

// Depth2DepthTransform on all tiles (channel 0), in place.
__global__ void __launch_bounds__(kBlock) k_apply_cubic(const TileGeom* __restrict__ geom,
                                                        int ntiles, float* __restrict__ tiles,
                                                        long long tstride,
                                                        const float* __restrict__ coeffs)
{
    const int p = blockIdx.y, b = blockIdx.z;
    const TileGeom g = geom[p];
    long long npx = (long long)g.w * g.h;
    const float4 abcd = *reinterpret_cast<const float4*>(coeffs + ((long long)b * ntiles + p) * 4);
    float* t = tiles + b * tstride + g.off;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < npx;
         i += (long long)gridDim.x * kBlock)
        t[i * g.c] = cubic_map(t[i * g.c], abcd.x, abcd.y, abcd.z, abcd.w);
}

// The same under the validity rule: a valid pixel is transformed, an invalid one becomes a quiet
// NaN (and so stays invalid under any later lo / hi).
__global__ void __launch_bounds__(kBlock) k_apply_cubic_valid(const TileGeom* __restrict__ geom,
                                                              int ntiles,
                                                              float* __restrict__ tiles,
                                                              long long tstride,
                                                              const float* __restrict__ coeffs,
                                                              float vlo, float vhi)
{
    const int p = blockIdx.y, b = blockIdx.z;
    const TileGeom g = geom[p];
    long long npx = (long long)g.w * g.h;
    const float4 abcd = *reinterpret_cast<const float4*>(coeffs + ((long long)b * ntiles + p) * 4);
    float* t = tiles + b * tstride + g.off;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < npx;
         i += (long long)gridDim.x * kBlock) {
        const float v = t[i * g.c];
        t[i * g.c] = tile_ok(v, vlo, vhi) ? cubic_map(v, abcd.x, abcd.y, abcd.z, abcd.w)
                                          : __uint_as_float(0x7FC00000u);
    }
}

// ---- planar-depth tiles (pf_set_tile_depth) ---------------------------------------------------
// pf_tile_ray_factor: kf of every tile pixel, layout order (one float per pixel, no channels).
__global__ void __launch_bounds__(kBlock) k_ray_factor(const TileGeom* __restrict__ geom,
                                                       const RayTile* __restrict__ ray,
                                                       const double* __restrict__ tab,
                                                       float* __restrict__ out)
{
    const int p = blockIdx.y;
    const TileGeom g = geom[p];
    const RayTile rt = ray[p];
    const int npx = g.w * g.h;
    float* o = out + g.pix_off;
    // i stays below npx <= INT32_MAX inside the loop; the 64-bit counter only keeps the stride add
    // from wrapping
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < npx;
         i += (long long)gridDim.x * kBlock)
        o[i] = ray_kf(tab, rt, (int)i % g.w, (int)i / g.w);
}

// The registration samples' ray factor, next to their indices (k_regidx): sample s of tile p reads
// tile element sidx[s].x, i.e. pixel sidx[s].x / c.  Layout- and baseline-size-only, built once,
// so the sample-wise solvers' 8-27 passes load a float instead of taking an fp64 sqrt.
__global__ void __launch_bounds__(256) k_reg_kf(const TileGeom* __restrict__ geom,
                                                const RegGrid* __restrict__ grids,
                                                const RayTile* __restrict__ ray,
                                                const double* __restrict__ tab,
                                                const int2* __restrict__ sidx,
                                                float* __restrict__ kfs)
{
    const int p = blockIdx.y;
    const TileGeom g = geom[p];
    const RegGrid rg = grids[p];
    const RayTile rt = ray[p];
    const int ns = (rg.cols + 1) * (rg.rows + 1);
    for (int s = blockIdx.x * 256 + threadIdx.x; s < ns; s += gridDim.x * 256) {
        const int pix = sidx[rg.soff + s].x / g.c;
        kfs[rg.soff + s] = ray_kf(tab, rt, pix % g.w, pix / g.w);
    }
}

// Depth2DepthTransform composed with the ray factor, src -> dst (in place when they are equal):
// clamp01(kf * T32(X)), T32 = cubic_map's fp32 value before its final clamp, in its operation
// order; one fp32 multiply by kf (the unit is built without contraction); NaN stays NaN.  VALID:
// a pixel that fails the rule becomes a quiet NaN.
template <bool VALID>
__device__ __forceinline__ void apply_cubic_planar(const TileGeom* __restrict__ geom,
                                                   const RayTile* __restrict__ ray,
                                                   const double* __restrict__ tab, int ntiles,
                                                   const float* src, float* dst, long long tstride,
                                                   const float* __restrict__ coeffs, float vlo,
                                                   float vhi)
{
    const int p = blockIdx.y, b = blockIdx.z;
    const TileGeom g = geom[p];
    const RayTile rt = ray[p];
    const int npx = g.w * g.h;
    const float4 abcd = *reinterpret_cast<const float4*>(coeffs + ((long long)b * ntiles + p) * 4);
    const float* in = src + b * tstride + g.off;
    float* t = dst + b * tstride + g.off;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < npx;
         i += (long long)gridDim.x * kBlock) {
        const float v = in[i * g.c];
        float X = v;
        if (X <= 9.99999974737875e-05f) X = (float)1e-4;  // cubic_map's clamps
        else if (X > 0.99989998340606689f) X = (float)(1 - 1e-4);
        float Y = abcd.x * X * X * X + abcd.y * X * X + abcd.z * X + abcd.w;
        Y = ray_kf(tab, rt, (int)i % g.w, (int)i / g.w) * Y;
        if (Y < 0) Y = 0;
        else if (Y > 1) Y = 1;
        if constexpr (VALID)
            if (!tile_ok(v, vlo, vhi)) Y = __uint_as_float(0x7FC00000u);
        t[i * g.c] = Y;
    }
}

__global__ void __launch_bounds__(kBlock) k_apply_cubic_planar(
    const TileGeom* __restrict__ geom, const RayTile* __restrict__ ray,
    const double* __restrict__ tab, int ntiles, const float* src, float* dst, long long tstride,
    const float* __restrict__ coeffs)
{
    apply_cubic_planar<false>(geom, ray, tab, ntiles, src, dst, tstride, coeffs, 0.0f, 0.0f);
}

__global__ void __launch_bounds__(kBlock) k_apply_cubic_planar_valid(
    const TileGeom* __restrict__ geom, const RayTile* __restrict__ ray,
    const double* __restrict__ tab, int ntiles, const float* src, float* dst, long long tstride,
    const float* __restrict__ coeffs, float vlo, float vhi)
{
    apply_cubic_planar<true>(geom, ray, tab, ntiles, src, dst, tstride, coeffs, vlo, vhi);
}

// Depth2DepthTransform of one map (PerspectiveMap::Depth2DepthTransform, Depth.cpp:245-274),
// channel 0 of every pixel, in place.
__global__ void __launch_bounds__(kBlock) k_d2d_map(float* __restrict__ data, long long npx,
                                                    int c, float a, float b, float cc, float d)
{
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < npx;
         i += (long long)gridDim.x * kBlock)
        data[i * c] = cubic_map(data[i * c], a, b, cc, d);
}

void launch_register(hipStream_t s, const TileGeom* geom, const RegGrid* grids,
                     const GridCol* rcols, const GridRow* rrows, int ntiles, const float* emap,
                     int ew, int eh, int ec, long long estride, const float* tiles,
                     long long tstride, int degree, int solver, float* coeffs, double* coeffs64,
                     int batch, double* sums, const int* active, const int2* sidx, TileValid tv)
{
    dim3 grid((unsigned)(ntiles * batch));
    if (tv.on)
        hipLaunchKernelGGL(k_register_valid, grid, dim3(kRegLanes), 0, s, geom, grids, rcols,
                           rrows, ntiles, emap, ew, eh, ec, estride, tiles, tstride, degree,
                           solver, coeffs, coeffs64, sums, active, sidx, tv.lo, tv.hi);
    else
        hipLaunchKernelGGL(k_register, grid, dim3(kRegLanes), 0, s, geom, grids, rcols, rrows,
                           ntiles, emap, ew, eh, ec, estride, tiles, tstride, degree, solver,
                           coeffs, coeffs64, sums, active, sidx);
}

void launch_register_weighted(hipStream_t s, const TileGeom* geom, const RegGrid* grids,
                              int ntiles, const float* emap, long long estride,
                              const float* tiles, long long tstride, const float* weights,
                              long long wstride, float* coeffs, double* coeffs64,
                              double* summary, int batch, const int2* sidx)
{
    hipLaunchKernelGGL(k_register_weighted, dim3((unsigned)(ntiles * batch)), dim3(kRegLanes), 0,
                       s, geom, grids, ntiles, emap, estride, tiles, tstride, weights, wstride,
                       coeffs, coeffs64, summary, sidx);
}

void launch_valid_counts(hipStream_t s, const TileGeom* geom, const RegGrid* grids, int ntiles,
                         const float* emap, long long estride, const float* tiles,
                         long long tstride, const int2* sidx, TileValid tv, long long* counts,
                         int batch)
{
    hipLaunchKernelGGL(k_valid_counts, dim3((unsigned)(ntiles * batch)), dim3(256), 0, s, geom,
                       grids, ntiles, emap, estride, tiles, tstride, sidx, tv, counts);
}

// One thread per registration sample: the tile element (SphericalTo2D, clamp, Value's index) and
// the baseline element (ValueAtCoord's index) of sample s of tile p, exactly as k_register's
// direct path computes them (Depth.cpp:1328-1387).
__global__ void __launch_bounds__(256) k_regidx(const TileGeom* __restrict__ geom,
                                                const RegGrid* __restrict__ grids,
                                                const GridCol* __restrict__ rcols,
                                                const GridRow* __restrict__ rrows, int ew, int eh,
                                                int ec, int2* __restrict__ sidx)
{
    const int p = blockIdx.y;
    const TileGeom g = geom[p];
    const RegGrid rg = grids[p];
    const int ncol = rg.cols + 1;
    const int ns = ncol * (rg.rows + 1);
    for (int s = blockIdx.x * 256 + threadIdx.x; s < ns; s += gridDim.x * 256) {
        const int r = s / ncol, c = s - r * ncol;
        const GridCol cc = rcols[rg.col_off + c];
        const GridRow rr = rrows[rg.row_off + r];
        float x, y;
        sph_to_2d(g, rr.sz, rr.cz, cc.ca, cc.sa, x, y);
        if (x < 0) x = 0;
        if (x > 1) x = 1;
        if (y < 0) y = 0;
        if (y > 1) y = 1;
        sidx[rg.soff + s] = make_int2((int)tile_index(g, x, y),
                                      (int)emap_index(cc.az, rr.zen, ew, eh, ec));
    }
}

void launch_regidx(hipStream_t s, const TileGeom* geom, const RegGrid* grids,
                   const GridCol* rcols, const GridRow* rrows, int ntiles, int max_samples,
                   int ew, int eh, int ec, int2* sidx)
{
    unsigned gx = (unsigned)((max_samples + 255) / 256);
    if (gx < 1) gx = 1;
    if (gx > 1024) gx = 1024;
    hipLaunchKernelGGL(k_regidx, dim3(gx, (unsigned)ntiles), dim3(256), 0, s, geom, grids, rcols,
                       rrows, ew, eh, ec, sidx);
}

int register_sums_per_tile() { return kRegSums; }

// SolveDepthToDepth2's solve (Depth.cpp:1158-1259): per panorama, the chunk partials of
// k_global_sums (pf_global.hip) added in chunk order from 0.0, then the LM from (0, 0, 1, 0).
// One wave per panorama: lane k < 15 adds sum k over the chunks (eight loads in flight, added in
// chunk order), lane 0 solves.
__global__ void __launch_bounds__(64) k_global_solve(const double* __restrict__ partials,
                                                     int nchunks, int batch,
                                                     float* __restrict__ coeffs,
                                                     double* __restrict__ coeffs64,
                                                     double* __restrict__ summary)
{
    __shared__ double Ssh[kRegSums];
    const int b = blockIdx.x, k = threadIdx.x;
    if (k < kRegSums) {
        const double* p = partials + (long long)b * nchunks * kRegSums + k;
        double acc = 0.0;
        for (int c0 = 0; c0 < nchunks; c0 += 8) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; u++)
                v[u] = c0 + u < nchunks ? p[(long long)(c0 + u) * kRegSums] : 0.0;
#pragma unroll
            for (int u = 0; u < 8; u++)
                if (c0 + u < nchunks) acc = acc + v[u];
        }
        Ssh[k] = acc;
    }
    __syncthreads();
    if (k != 0) return;
    double S[kRegSums];
    for (int i = 0; i < kRegSums; i++) S[i] = Ssh[i];
    const double start[4] = {0.0, 0.0, 1.0, 0.0};
    double c[4], sm[4];
    lm_moments(S, start, c, sm);
    for (int i = 0; i < 4; i++) {
        if (coeffs) coeffs[(long long)b * 4 + i] = (float)c[i];  // Vec4f(vars), Depth.cpp:1251
        if (coeffs64) coeffs64[(long long)b * 4 + i] = c[i];
        if (summary) summary[(long long)b * 4 + i] = sm[i];
    }
}

void launch_global_solve(hipStream_t s, const double* partials, int nchunks, int batch,
                         float* coeffs, double* coeffs64, double* summary)
{
    hipLaunchKernelGGL(k_global_solve, dim3((unsigned)batch), dim3(64), 0, s, partials, nchunks,
                       batch, coeffs, coeffs64, summary);
}

void launch_register_joint(hipStream_t s, const double* sums, const int* active, int ntiles,
                           int batch, int degree, int solver, float* coeffs, double* coeffs64,
                           bool guard)
{
    hipLaunchKernelGGL(k_register_joint, dim3((batch + 63) / 64), dim3(64), 0, s, sums, active,
                       ntiles, batch, degree, solver, coeffs, coeffs64, guard ? 1 : 0);
}

void launch_apply_cubic(hipStream_t s, const TileGeom* geom, int ntiles, long long tile_elems,
                        float* tiles, long long tstride, const float* coeffs, int batch,
                        TileValid tv)
{
    long long per = tile_elems / (ntiles > 0 ? ntiles : 1);
    unsigned gx = nblocks(per);
    if (gx > 1024) gx = 1024;
    if (gx == 0) gx = 1;
    dim3 grid(gx, ntiles, batch);
    if (tv.on)
        hipLaunchKernelGGL(k_apply_cubic_valid, grid, dim3(kBlock), 0, s, geom, ntiles, tiles,
                           tstride, coeffs, tv.lo, tv.hi);
    else
        hipLaunchKernelGGL(k_apply_cubic, grid, dim3(kBlock), 0, s, geom, ntiles, tiles, tstride,
                           coeffs);
}

void launch_register_planar(hipStream_t s, const TileGeom* geom, const RegGrid* grids, int ntiles,
                            const float* emap, long long estride, const float* tiles,
                            long long tstride, int degree, int solver, float* coeffs,
                            double* coeffs64, int batch, const int2* sidx, const float* kfs,
                            TileValid tv)
{
    dim3 grid((unsigned)(ntiles * batch));
    if (tv.on)
        hipLaunchKernelGGL(k_register_planar_valid, grid, dim3(kRegLanes), 0, s, geom, grids,
                           ntiles, emap, estride, tiles, tstride, degree, solver, coeffs, coeffs64,
                           sidx, kfs, tv.lo, tv.hi);
    else
        hipLaunchKernelGGL(k_register_planar, grid, dim3(kRegLanes), 0, s, geom, grids, ntiles,
                           emap, estride, tiles, tstride, degree, solver, coeffs, coeffs64, sidx,
                           kfs);
}

static unsigned pixel_blocks(long long tile_pixels, int ntiles)
{
    unsigned gx = nblocks(tile_pixels / (ntiles > 0 ? ntiles : 1));
    if (gx > 1024) gx = 1024;
    if (gx == 0) gx = 1;
    return gx;
}

void launch_ray_factor(hipStream_t s, const TileGeom* geom, const RayTile* ray, const double* tab,
                       int ntiles, long long tile_pixels, float* out)
{
    hipLaunchKernelGGL(k_ray_factor, dim3(pixel_blocks(tile_pixels, ntiles), ntiles), dim3(kBlock),
                       0, s, geom, ray, tab, out);
}

void launch_reg_kf(hipStream_t s, const TileGeom* geom, const RegGrid* grids, const RayTile* ray,
                   const double* tab, int ntiles, int max_samples, const int2* sidx, float* kfs)
{
    unsigned gx = (unsigned)((max_samples + 255) / 256);
    if (gx < 1) gx = 1;
    if (gx > 1024) gx = 1024;
    hipLaunchKernelGGL(k_reg_kf, dim3(gx, (unsigned)ntiles), dim3(256), 0, s, geom, grids, ray,
                       tab, sidx, kfs);
}

void launch_apply_cubic_planar(hipStream_t s, const TileGeom* geom, const RayTile* ray,
                               const double* tab, int ntiles, long long tile_pixels,
                               const float* src, float* dst, long long tstride,
                               const float* coeffs, int batch, TileValid tv)
{
    dim3 grid(pixel_blocks(tile_pixels, ntiles), ntiles, batch);
    if (tv.on)
        hipLaunchKernelGGL(k_apply_cubic_planar_valid, grid, dim3(kBlock), 0, s, geom, ray, tab,
                           ntiles, src, dst, tstride, coeffs, tv.lo, tv.hi);
    else
        hipLaunchKernelGGL(k_apply_cubic_planar, grid, dim3(kBlock), 0, s, geom, ray, tab, ntiles,
                           src, dst, tstride, coeffs);
}

void launch_d2d_map(hipStream_t s, float* data, long long npx, int c, const float* abcd)
{
    unsigned gx = nblocks(npx);
    if (gx > 4096) gx = 4096;
    if (gx == 0) gx = 1;
    hipLaunchKernelGGL(k_d2d_map, dim3(gx), dim3(kBlock), 0, s, data, npx, c, abcd[0], abcd[1],
                       abcd[2], abcd[3]);
}


}  // namespace pf
