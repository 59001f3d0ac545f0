// pf_robust.hip -- robust cubic tile registration (pf_set_register_loss): the per-tile fit of
// y = a x^3 + b x^2 + c x + d under Ceres 1.13's HuberLoss or SoftLOneLoss, by the reference's
// trust-region Levenberg-Marquardt (lm_solve, pf_lm.hpp).
//
// k_register solves the cubic from 15 moment sums; a loss weights every sample by a function of
// its own residual, which moments cannot carry, so this kernel is sample-wise, in the form of
// k_register_disp (pf_disp.hip): one 256-lane workgroup owns one (panorama, tile) pair, gathers the
// samples once through the cached indices, keeps up to 32 (x, y) float pairs per lane in
// registers, and runs the whole LM on them.  A Jacobian evaluation reduces 15 fp64 sums (cost, 4
// of J'r, 10 of upper J'J, all of the corrected residual sqrt(rho') r and row sqrt(rho') J), a
// trial evaluation 1.  Every lane runs the scalar LM algebra on the same reduced sums, so every
// branch is block-uniform; blocks never talk to each other.
//
// Summation order (part of the contract; tests/robust_ref.py restates it): lane l adds its samples
// l, l + 256, ... in order from 0.0, then the halving tree of disp_reduce.  Only fp64 + - * / sqrt,
// no contraction.  LDS: 15 x 256 doubles (+ 15 totals).
#include "pf_lm.hpp"

namespace pf {

namespace {
constexpr int kRobSums = 15;  // cost, J'r (4), upper J'J (10, row-major)

// One sample's residual at p = (a, b, c, d), and its powers: the Jacobian row is (X3, X2, X, 1).
__device__ __forceinline__ double cubic_residual(double X, double Y, const double p[4], double& X2,
                                                 double& X3)
{
    X2 = X * X;
    X3 = X * X * X;
    return (((X3 * p[0] + X2 * p[1]) + X * p[2]) + p[3]) - Y;
}

// The same for a planar-depth tile (pf_set_tile_depth): the model is K times the cubic, K the
// sample's ray factor, so r = K m - Y and the row is (K X3, K X2, K X, K).
__device__ __forceinline__ double planar_residual(double X, double Y, double K, const double p[4],
                                                  double& X2, double& X3)
{
    X2 = X * X;
    X3 = X * X * X;
    return K * (((X3 * p[0] + X2 * p[1]) + X * p[2]) + p[3]) - Y;
}

template <bool PLANAR>
__device__ __forceinline__ void rob_terms(double X, double Y, double K, const double p[4],
                                          double acc[kRobSums], const RegLoss& L)
{
    double X2, X3, rho0, rho1;
    const double r = PLANAR ? planar_residual(X, Y, K, p, X2, X3) : cubic_residual(X, Y, p, X2, X3);
    loss_eval(L, r * r, rho0, rho1);
    const double w = sqrt(rho1);
    const double rc = w * r;
    double j0, j1, j2, j3;
    if constexpr (PLANAR) {
        j0 = w * (K * X3);
        j1 = w * (K * X2);
        j2 = w * (K * X);
        j3 = w * K;
    } else {
        j0 = w * X3;
        j1 = w * X2;
        j2 = w * X;
        j3 = w;
    }
    acc[0] = acc[0] + 0.5 * rho0;
    acc[1] = acc[1] + j0 * rc;
    acc[2] = acc[2] + j1 * rc;
    acc[3] = acc[3] + j2 * rc;
    acc[4] = acc[4] + j3 * rc;
    acc[5] = acc[5] + j0 * j0;
    acc[6] = acc[6] + j0 * j1;
    acc[7] = acc[7] + j0 * j2;
    acc[8] = acc[8] + j0 * j3;
    acc[9] = acc[9] + j1 * j1;
    acc[10] = acc[10] + j1 * j2;
    acc[11] = acc[11] + j1 * j3;
    acc[12] = acc[12] + j2 * j2;
    acc[13] = acc[13] + j2 * j3;
    acc[14] = acc[14] + j3 * j3;
}

template <bool PLANAR>
__device__ __forceinline__ void rob_cost_term(double X, double Y, double K, const double p[4],
                                              double& acc, const RegLoss& L)
{
    double X2, X3, rho0, rho1;
    const double r = PLANAR ? planar_residual(X, Y, K, p, X2, X3) : cubic_residual(X, Y, p, X2, X3);
    loss_eval(L, r * r, rho0, rho1);
    acc = acc + 0.5 * rho0;
}
}  // namespace

// MASK: under the validity rule (k_register_valid's: a sample whose raw tile value fails the rule,
// or whose baseline value is not finite, is skipped and adds nothing).
// PLANAR (k_register_robust_planar): with the samples' ray factor kfs (k_reg_kf).  The resident
// registers hold (x, y) as before -- a third resident value per sample does not fit beside them --
// and K is a float load from the cached table in every pass (coalesced: lane l reads
// kfs[l + 256 u]), widened to fp64.  The lane-to-sample order is unchanged.
template <bool MASK, bool PLANAR>
__device__ __forceinline__ void register_robust_tile(
    const TileGeom* __restrict__ geom, const RegGrid* __restrict__ grids, int ntiles,
    const float* __restrict__ emap, long long estride, const float* __restrict__ tiles,
    long long tstride, const int2* __restrict__ sidx, const float* __restrict__ kfs,
    float* __restrict__ coeffs, double* __restrict__ coeffs64, double* __restrict__ summary,
    const RegLoss L, float vlo, float vhi, double (*part)[kDispLanes], double* tot)
{
    // k_register_disp's block order: the tiles of one panorama on one XCD
    const unsigned lb = xcd_remap(blockIdx.x, gridDim.x);
    const int p = (int)(lb % (unsigned)ntiles), b = (int)(lb / (unsigned)ntiles), l = threadIdx.x;
    const RegGrid rg = grids[p];
    const float* tile = tiles + b * tstride + geom[p].off;
    const float* em = emap + b * estride;
    const int2* ix = sidx + rg.soff;
    const int ns = (rg.cols + 1) * (rg.rows + 1);
    const float* kf = PLANAR ? kfs + rg.soff : nullptr;
    auto Kof = [&](int s) { return PLANAR ? (double)kf[s] : 1.0; };
    auto kept = [&](float tv, float ev) {
        if constexpr (MASK) return tile_ok(tv, vlo, vhi) && isfinite(ev);
        return true;
    };

    // the lane's resident samples l, l + 256, ...: gathered once (independent loads); bit u of
    // live: sample u exists and is kept
    float xs[kDispPerLane], ys[kDispPerLane];
    unsigned live = 0u;
#pragma unroll
    for (int u = 0; u < kDispPerLane; u++) {
        const int s = l + u * kDispLanes;
        xs[u] = 0.5f;
        ys[u] = 0.5f;
        if (s < ns) {
            const int2 i2 = ix[s];
            xs[u] = tile[i2.x];
            ys[u] = em[i2.y];
            if (kept(xs[u], ys[u])) live |= 1u << u;
        }
    }

    // each(f): f(X, Y, K) on the lane's kept samples in order, X and Y clamped in fp64 (K: the
    // constant 1.0, unused, without PLANAR).  The empty
    // asm keeps the compiler from widening the 64 resident floats to clamped doubles once and
    // holding those across the evaluations: that form spills to scratch.
    auto each = [&](auto&& f) {
#pragma unroll
        for (int u = 0; u < kDispPerLane; u++)
            if (live >> u & 1u) {
                float xv = xs[u], yv = ys[u];
                asm volatile("" : "+v"(xv), "+v"(yv));
                f(clamp_sample((double)xv), clamp_sample((double)yv), Kof(l + u * kDispLanes));
            }
        for (int s = l + kDispResident; s < ns; s += kDispLanes) {  // past the capacity
            const int2 i2 = ix[s];
            const float tv = tile[i2.x], ev = em[i2.y];
            if (kept(tv, ev)) f(clamp_sample((double)tv), clamp_sample((double)ev), Kof(s));
        }
    };
    auto eval_full = [&](const double (&q)[4], double& cost, double (&g)[4], double (&M)[4][4]) {
        double S[kRobSums];
#pragma unroll
        for (int k = 0; k < kRobSums; k++) S[k] = 0.0;
        each([&](double X, double Y, double K) { rob_terms<PLANAR>(X, Y, K, q, S, L); });
        disp_reduce<kRobSums>(S, part, tot, l);
        cost = S[0];
        int at = 5;  // upper J'J, row-major
        for (int i = 0; i < 4; i++) {
            g[i] = S[1 + i];
            for (int j = i; j < 4; j++) M[i][j] = M[j][i] = S[at++];
        }
    };
    auto eval_cost = [&](const double (&q)[4]) {
        double c = 0.0;
        each([&](double X, double Y, double K) { rob_cost_term<PLANAR>(X, Y, K, q, c, L); });
        disp_reduce<1>(&c, part, tot, l);
        return c;
    };

    const long long o = (long long)b * ntiles + p;
    const double qnan = __longlong_as_double(0x7FF8000000000000LL);
    double used = (double)ns;
    if constexpr (MASK) {
        used = 0.0;
        each([&](double, double, double) { used = used + 1.0; });
        disp_reduce<1>(&used, part, tot, l);
        if (used < 4.0) {  // block-uniform: too few samples for the four coefficients
            if (l == 0) {
                for (int i = 0; i < 4; i++) {
                    if (coeffs) coeffs[o * 4 + i] = __uint_as_float(0x7FC00000u);
                    if (coeffs64) coeffs64[o * 4 + i] = qnan;
                }
                if (summary) {
                    summary[o * 6 + 0] = qnan;
                    summary[o * 6 + 1] = qnan;
                    summary[o * 6 + 2] = 0.0;
                    summary[o * 6 + 3] = (double)kTermFailure;
                    summary[o * 6 + 4] = used;
                    summary[o * 6 + 5] = 0.0;
                }
            }
            return;
        }
    }

    // lm_solve (pf_lm.hpp) for four parameter blocks: DENSE_SCHUR eliminates a, the reduced system
    // is 3x3 in (b, c, d).  Every lane holds the same sums, hence the same state.
    const double start[4] = {1.0, 1.0, 1.0, 1.0};  // Depth.cpp:1270-1274
    double best[4];
    LmSummary sm;
    lm_solve<4, true>(start, eval_full, eval_cost, best, sm);

    // one more pass at the returned parameters: the samples with r r <= a a (exact counts)
    double inliers = 0.0;
    each([&](double X, double Y, double K) {
        double X2, X3;
        const double r =
            PLANAR ? planar_residual(X, Y, K, best, X2, X3) : cubic_residual(X, Y, best, X2, X3);
        if (r * r <= L.b) inliers = inliers + 1.0;
    });
    disp_reduce<1>(&inliers, part, tot, l);
    if (l == 0) {
        bool finite = true;
        for (int i = 0; i < 4; i++) finite = finite && isfinite(best[i]);
        if (!finite) sm.termination = kTermFailure;
        for (int i = 0; i < 4; i++) {
            if (coeffs)  // Vec4f(vars), Depth.cpp:1408
                coeffs[o * 4 + i] = finite ? (float)best[i] : __uint_as_float(0x7FC00000u);
            if (coeffs64) coeffs64[o * 4 + i] = finite ? best[i] : qnan;
        }
        if (summary) {
            summary[o * 6 + 0] = sm.initial_cost;
            summary[o * 6 + 1] = sm.final_cost;
            summary[o * 6 + 2] = (double)sm.iterations;
            summary[o * 6 + 3] = (double)sm.termination;
            summary[o * 6 + 4] = used;
            summary[o * 6 + 5] = inliers;
        }
    }
}

template <bool MASK>
__global__ void __launch_bounds__(kDispLanes) k_register_robust(
    const TileGeom* __restrict__ geom, const RegGrid* __restrict__ grids, int ntiles,
    const float* __restrict__ emap, long long estride, const float* __restrict__ tiles,
    long long tstride, const int2* __restrict__ sidx, float* __restrict__ coeffs,
    double* __restrict__ coeffs64, double* __restrict__ summary, RegLoss L, float vlo, float vhi)
{
    __shared__ double part[kRobSums][kDispLanes];
    __shared__ double tot[kRobSums];
    register_robust_tile<MASK, false>(geom, grids, ntiles, emap, estride, tiles, tstride, sidx,
                                      nullptr, coeffs, coeffs64, summary, L, vlo, vhi, part, tot);
}

template <bool MASK>
__global__ void __launch_bounds__(kDispLanes) k_register_robust_planar(
    const TileGeom* __restrict__ geom, const RegGrid* __restrict__ grids, int ntiles,
    const float* __restrict__ emap, long long estride, const float* __restrict__ tiles,
    long long tstride, const int2* __restrict__ sidx, const float* __restrict__ kfs,
    float* __restrict__ coeffs, double* __restrict__ coeffs64, double* __restrict__ summary,
    RegLoss L, float vlo, float vhi)
{
    __shared__ double part[kRobSums][kDispLanes];
    __shared__ double tot[kRobSums];
    register_robust_tile<MASK, true>(geom, grids, ntiles, emap, estride, tiles, tstride, sidx, kfs,
                                     coeffs, coeffs64, summary, L, vlo, vhi, part, tot);
}

void launch_register_robust_planar(hipStream_t s, const TileGeom* geom, const RegGrid* grids,
                                   int ntiles, const float* emap, long long estride,
                                   const float* tiles, long long tstride, const int2* sidx,
                                   const float* kfs, float* coeffs, double* coeffs64,
                                   double* summary, int batch, int loss_kind, double loss_a,
                                   TileValid tv)
{
    const dim3 grid((unsigned)(ntiles * batch)), block(kDispLanes);
    const RegLoss L = make_loss(loss_kind, loss_a);
    if (tv.on)
        hipLaunchKernelGGL(k_register_robust_planar<true>, grid, block, 0, s, geom, grids, ntiles,
                           emap, estride, tiles, tstride, sidx, kfs, coeffs, coeffs64, summary, L,
                           tv.lo, tv.hi);
    else
        hipLaunchKernelGGL(k_register_robust_planar<false>, grid, block, 0, s, geom, grids,
                           ntiles, emap, estride, tiles, tstride, sidx, kfs, coeffs, coeffs64,
                           summary, L, 0.0f, 0.0f);
}

void launch_register_robust(hipStream_t s, const TileGeom* geom, const RegGrid* grids, int ntiles,
                            const float* emap, long long estride, const float* tiles,
                            long long tstride, const int2* sidx, float* coeffs, double* coeffs64,
                            double* summary, int batch, int loss_kind, double loss_a, TileValid tv)
{
    const dim3 grid((unsigned)(ntiles * batch)), block(kDispLanes);
    const RegLoss L = make_loss(loss_kind, loss_a);
    if (tv.on)
        hipLaunchKernelGGL(k_register_robust<true>, grid, block, 0, s, geom, grids, ntiles, emap,
                           estride, tiles, tstride, sidx, coeffs, coeffs64, summary, L, tv.lo,
                           tv.hi);
    else
        hipLaunchKernelGGL(k_register_robust<false>, grid, block, 0, s, geom, grids, ntiles, emap,
                           estride, tiles, tstride, sidx, coeffs, coeffs64, summary, L, 0.0f,
                           0.0f);
}

}  // namespace pf
