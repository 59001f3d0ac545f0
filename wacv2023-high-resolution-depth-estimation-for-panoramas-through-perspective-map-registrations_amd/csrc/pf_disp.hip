// pf_disp.hip -- disparity-tile registration: the per-tile fit of y = 1/(a x + b) + d
// (FunctorDisparity2Depth, Depth.cpp:1044-1073) by the reference's Ceres 1.13 trust-region
// Levenberg-Marquardt (lm_solve, pf_lm.hpp), and PerspectiveMap::D2DTransform (Depth.cpp:214-243).
//
// The cubic of k_register is linear in its coefficients, so its LM runs on 15 moment sums.  This
// model is not: every LM evaluation is a pass over the tile's samples.  One 256-lane workgroup
// owns one (panorama, tile) pair, gathers the samples once, keeps them in registers (up to a capacity), and runs the
// whole LM on them: a Jacobian evaluation reduces 10 fp64 sums, a trial evaluation 1.  Every lane
// runs the (scalar) LM algebra on the same reduced sums, so every branch is block-uniform; blocks
// never talk to each other.
//
// Summation order (part of the contract; tests/disp_ref.py restates it): lane l adds its samples
// l, l + 256, ... in order from 0.0, then the halving tree of k_register (stride 128, 64, ..., 1:
// p[l] = p[l] + p[l + stride]).  Only fp64 + - * / sqrt, no contraction.
#include "pf_lm.hpp"

namespace pf {

namespace {
constexpr int kDispSums = 10;  // cost, J'r (3), upper J'J (6)

// One sample's terms at p = (a, b, d): r = (q + d) - Y with q = 1 / (a X + b), Jacobian row
// (-(X q q), -(q q), 1).
// With LOSS (pf_set_register_loss) the cost term is 0.5 rho(r r) and the residual and the row
// are scaled by sqrt(rho'(r r)) first (pf_lm.hpp); without, this is the code it always was.
// PLANAR (pf_set_tile_depth): the model is K (q + d) with the sample's ray factor K, so
// r = K (q + d) - Y and the row is (K j0, K j1, K), one multiply per entry, before any loss.
template <bool LOSS, bool PLANAR = false>
__device__ __forceinline__ void disp_terms(double X, double Y, const double p[3],
                                           double acc[kDispSums], const RegLoss& L, double K = 1.0)
{
    const double q = 1.0 / (p[0] * X + p[1]);
    const double qq = q * q;
    if constexpr (PLANAR) {
        const double r = K * (q + p[2]) - Y;
        double k0 = K * -(X * qq), k1 = K * -qq, k2 = K, rc = r, c0 = 0.5 * (r * r);
        if constexpr (LOSS) {
            double rho0, rho1;
            loss_eval(L, r * r, rho0, rho1);
            const double w = sqrt(rho1);
            rc = w * r;
            k0 = w * k0;
            k1 = w * k1;
            k2 = w * k2;
            c0 = 0.5 * rho0;
        }
        acc[0] = acc[0] + c0;
        acc[1] = acc[1] + k0 * rc;
        acc[2] = acc[2] + k1 * rc;
        acc[3] = acc[3] + k2 * rc;
        acc[4] = acc[4] + k0 * k0;
        acc[5] = acc[5] + k0 * k1;
        acc[6] = acc[6] + k0 * k2;
        acc[7] = acc[7] + k1 * k1;
        acc[8] = acc[8] + k1 * k2;
        acc[9] = acc[9] + k2 * k2;
        return;
    }
    const double r = (q + p[2]) - Y;
    const double j0 = -(X * qq), j1 = -qq;
    if constexpr (LOSS) {
        double rho0, rho1;
        loss_eval(L, r * r, rho0, rho1);
        const double w = sqrt(rho1);
        const double rc = w * r, k0 = w * j0, k1 = w * j1, k2 = w;
        acc[0] = acc[0] + 0.5 * rho0;
        acc[1] = acc[1] + k0 * rc;
        acc[2] = acc[2] + k1 * rc;
        acc[3] = acc[3] + k2 * rc;
        acc[4] = acc[4] + k0 * k0;
        acc[5] = acc[5] + k0 * k1;
        acc[6] = acc[6] + k0 * k2;
        acc[7] = acc[7] + k1 * k1;
        acc[8] = acc[8] + k1 * k2;
        acc[9] = acc[9] + k2 * k2;
        return;
    }
    acc[0] = acc[0] + 0.5 * (r * r);
    acc[1] = acc[1] + j0 * r;
    acc[2] = acc[2] + j1 * r;
    acc[3] = acc[3] + r;
    acc[4] = acc[4] + j0 * j0;
    acc[5] = acc[5] + j0 * j1;
    acc[6] = acc[6] + j0;
    acc[7] = acc[7] + j1 * j1;
    acc[8] = acc[8] + j1;
    acc[9] = acc[9] + 1.0;
}

template <bool LOSS, bool PLANAR = false>
__device__ __forceinline__ void disp_cost_term(double X, double Y, const double p[3], double& acc,
                                               const RegLoss& L, double K = 1.0)
{
    const double q = 1.0 / (p[0] * X + p[1]);
    const double r = PLANAR ? K * (q + p[2]) - Y : (q + p[2]) - Y;
    if constexpr (LOSS) {
        double rho0, rho1;
        loss_eval(L, r * r, rho0, rho1);
        acc = acc + 0.5 * rho0;
        return;
    }
    acc = acc + 0.5 * (r * r);
}

// The weighted form (pf_register_disparity_weighted): W times each of disp_terms' ten terms in
// their order, multiply and add apart, so W = 1.0 leaves every bit of the unweighted sums.
template <bool PLANAR>
__device__ __forceinline__ void disp_terms_weighted(double X, double Y, double W,
                                                    const double p[3], double acc[kDispSums],
                                                    double K)
{
    const double q = 1.0 / (p[0] * X + p[1]);
    const double qq = q * q;
    if constexpr (PLANAR) {
        const double r = K * (q + p[2]) - Y;
        const double k0 = K * -(X * qq), k1 = K * -qq, k2 = K;
        acc[0] = acc[0] + W * (0.5 * (r * r));
        acc[1] = acc[1] + W * (k0 * r);
        acc[2] = acc[2] + W * (k1 * r);
        acc[3] = acc[3] + W * (k2 * r);
        acc[4] = acc[4] + W * (k0 * k0);
        acc[5] = acc[5] + W * (k0 * k1);
        acc[6] = acc[6] + W * (k0 * k2);
        acc[7] = acc[7] + W * (k1 * k1);
        acc[8] = acc[8] + W * (k1 * k2);
        acc[9] = acc[9] + W * (k2 * k2);
        return;
    }
    const double r = (q + p[2]) - Y;
    const double j0 = -(X * qq), j1 = -qq;
    acc[0] = acc[0] + W * (0.5 * (r * r));
    acc[1] = acc[1] + W * (j0 * r);
    acc[2] = acc[2] + W * (j1 * r);
    acc[3] = acc[3] + W * r;
    acc[4] = acc[4] + W * (j0 * j0);
    acc[5] = acc[5] + W * (j0 * j1);
    acc[6] = acc[6] + W * j0;
    acc[7] = acc[7] + W * (j1 * j1);
    acc[8] = acc[8] + W * j1;
    acc[9] = acc[9] + W * 1.0;
}

template <bool PLANAR>
__device__ __forceinline__ void disp_cost_term_weighted(double X, double Y, double W,
                                                        const double p[3], double& acc, double K)
{
    const double q = 1.0 / (p[0] * X + p[1]);
    const double r = PLANAR ? K * (q + p[2]) - Y : (q + p[2]) - Y;
    acc = acc + W * (0.5 * (r * r));
}
}  // namespace

// One block's fit of tile p of panorama b.  LOSS: under the robust loss L, with the 6-entry
// summary of pf_register_ex; without, k_register_disp as it was.  PLANAR: with the samples' ray
// factor kfs (k_reg_kf).  The resident registers hold (x, y) as before; K is a float load from the
// cached table in every pass (coalesced: lane l reads kfs[l + 256 u]), widened to fp64 -- a third
// resident value per sample does not fit the register file, and the load replaces nothing that
// was in registers.  The lane-to-sample order is unchanged.
// WEIGHTED (pf_register_disparity_weighted; never with LOSS): ws is panorama b's row (wsstride
// floats each) of the usable sample weights (k_disp_sample_weights: u(w) of a used sample, 0.0f
// of any other), read like kfs in every pass: lane l reads ws[l + 256 u] and branches over a
// sample whose W is not > 0, so such a sample's terms (NaN, perhaps) are never formed.  The count
// of used samples and the sum of W are reduced first; fewer than 3 used samples, or a solution
// that is not finite, store quiet NaNs and termination 5.  Both decisions read block-reduced
// values: every exit is block-uniform.
template <bool LOSS, bool PLANAR = false, bool WEIGHTED = false>
__device__ __forceinline__ void register_disp_tile(
    const TileGeom* __restrict__ geom, const RegGrid* __restrict__ grids, int ntiles,
    const float* __restrict__ emap, long long estride, const float* __restrict__ tiles,
    long long tstride, const int2* __restrict__ sidx, float* __restrict__ coeffs,
    double* __restrict__ coeffs64, double* __restrict__ summary, const RegLoss L,
    double (*part)[kDispLanes], double* tot, const float* __restrict__ kfs = nullptr,
    const float* __restrict__ wsb = nullptr, long long wsstride = 0)
{
    static_assert(!(LOSS && WEIGHTED), "the weighted fit has no robust form");
    // k_register's block order: the tiles of one panorama on one XCD
    const unsigned lb = xcd_remap(blockIdx.x, gridDim.x);
    const int p = (int)(lb % (unsigned)ntiles), b = (int)(lb / (unsigned)ntiles), l = threadIdx.x;
    const RegGrid rg = grids[p];
    const float* tile = tiles + b * tstride + geom[p].off;
    const float* em = emap + b * estride;
    const int2* ix = sidx + rg.soff;
    const int ns = (rg.cols + 1) * (rg.rows + 1);
    const float* kf = PLANAR ? kfs + rg.soff : nullptr;
    auto Kof = [&](int s) { return PLANAR ? (double)kf[s] : 1.0; };
    const float* ws = WEIGHTED ? wsb + b * wsstride + rg.soff : nullptr;

    // the lane's resident samples l, l + 256, ...: gathered once (independent loads)
    float xs[kDispPerLane], ys[kDispPerLane];
#pragma unroll
    for (int u = 0; u < kDispPerLane; u++) {
        const int s = l + u * kDispLanes;
        xs[u] = 0.5f;
        ys[u] = 0.5f;
        if (s < ns) {
            const int2 i2 = ix[s];
            xs[u] = tile[i2.x];
            ys[u] = em[i2.y];
        }
    }

    auto eval_full = [&](const double (&q)[3], double& cost, double (&g)[3], double (&M)[3][3]) {
        double S[kDispSums];
#pragma unroll
        for (int k = 0; k < kDispSums; k++) S[k] = 0.0;
#pragma unroll
        for (int u = 0; u < kDispPerLane; u++)
            if (l + u * kDispLanes < ns) {
                if constexpr (WEIGHTED) {
                    const double W = (double)ws[l + u * kDispLanes];
                    if (W > 0.0)
                        disp_terms_weighted<PLANAR>(clamp_sample((double)xs[u]),
                                                    clamp_sample((double)ys[u]), W, q, S,
                                                    Kof(l + u * kDispLanes));
                } else {
                    disp_terms<LOSS, PLANAR>(clamp_sample((double)xs[u]),
                                             clamp_sample((double)ys[u]), q, S, L,
                                             Kof(l + u * kDispLanes));
                }
            }
        for (int s = l + kDispResident; s < ns; s += kDispLanes) {  // past the capacity
            if constexpr (WEIGHTED) {
                const double W = (double)ws[s];
                if (W > 0.0) {
                    const int2 i2 = ix[s];
                    disp_terms_weighted<PLANAR>(clamp_sample((double)tile[i2.x]),
                                                clamp_sample((double)em[i2.y]), W, q, S, Kof(s));
                }
                continue;
            }
            const int2 i2 = ix[s];
            disp_terms<LOSS, PLANAR>(clamp_sample((double)tile[i2.x]),
                                     clamp_sample((double)em[i2.y]), q, S, L, Kof(s));
        }
        disp_reduce<kDispSums>(S, part, tot, l);
        cost = S[0];
        for (int i = 0; i < 3; i++) g[i] = S[1 + i];
        M[0][0] = S[4];
        M[0][1] = M[1][0] = S[5];
        M[0][2] = M[2][0] = S[6];
        M[1][1] = S[7];
        M[1][2] = M[2][1] = S[8];
        M[2][2] = S[9];
    };
    auto eval_cost = [&](const double (&q)[3]) {
        double c = 0.0;
#pragma unroll
        for (int u = 0; u < kDispPerLane; u++)
            if (l + u * kDispLanes < ns) {
                if constexpr (WEIGHTED) {
                    const double W = (double)ws[l + u * kDispLanes];
                    if (W > 0.0)
                        disp_cost_term_weighted<PLANAR>(clamp_sample((double)xs[u]),
                                                        clamp_sample((double)ys[u]), W, q, c,
                                                        Kof(l + u * kDispLanes));
                } else {
                    disp_cost_term<LOSS, PLANAR>(clamp_sample((double)xs[u]),
                                                 clamp_sample((double)ys[u]), q, c, L,
                                                 Kof(l + u * kDispLanes));
                }
            }
        for (int s = l + kDispResident; s < ns; s += kDispLanes) {
            if constexpr (WEIGHTED) {
                const double W = (double)ws[s];
                if (W > 0.0) {
                    const int2 i2 = ix[s];
                    disp_cost_term_weighted<PLANAR>(clamp_sample((double)tile[i2.x]),
                                                    clamp_sample((double)em[i2.y]), W, q, c,
                                                    Kof(s));
                }
                continue;
            }
            const int2 i2 = ix[s];
            disp_cost_term<LOSS, PLANAR>(clamp_sample((double)tile[i2.x]),
                                         clamp_sample((double)em[i2.y]), q, c, L, Kof(s));
        }
        disp_reduce<1>(&c, part, tot, l);
        return c;
    };

    // lm_solve (pf_lm.hpp) for three parameter blocks: DENSE_SCHUR eliminates a, the reduced
    // system is 2x2 in (b, d).  Every lane holds the same sums, hence the same state.
    const double start[3] = {1.0, 1.0, 1.0};  // Depth.cpp:1270-1274
    double best[3];
    LmSummary sm;
    double used[2] = {0.0, 0.0};  // WEIGHTED: the used samples and the sum of W
    if constexpr (WEIGHTED) {
        for (int s = l; s < ns; s += kDispLanes) {
            const double W = (double)ws[s];
            if (W > 0.0) {
                used[0] = used[0] + 1.0;
                used[1] = used[1] + W;
            }
        }
        disp_reduce<2>(used, part, tot, l);
        if (used[0] < 3.0) {  // block-uniform: no fit
            if (l == 0) {
                const double qnan = __longlong_as_double(0x7FF8000000000000LL);
                const long long o = (long long)b * ntiles + p;
                for (int i = 0; i < 4; i++) {
                    if (coeffs) coeffs[o * 4 + i] = __uint_as_float(0x7FC00000u);
                    if (coeffs64) coeffs64[o * 4 + i] = qnan;
                }
                if (summary) {
                    summary[o * 6 + 0] = qnan;
                    summary[o * 6 + 1] = qnan;
                    summary[o * 6 + 2] = 0.0;
                    summary[o * 6 + 3] = (double)kTermFailure;
                    summary[o * 6 + 4] = used[0];
                    summary[o * 6 + 5] = used[1];
                }
            }
            return;
        }
    }
    lm_solve<3, true>(start, eval_full, eval_cost, best, sm);
    double inliers = 0.0;
    if constexpr (LOSS) {
        if (summary) {  // the samples with r r <= a a at the returned parameters (exact counts)
            auto count = [&](double X, double Y, double K) {
                const double m = 1.0 / (best[0] * X + best[1]) + best[2];
                const double r = PLANAR ? K * m - Y : m - Y;
                if (r * r <= L.b) inliers = inliers + 1.0;
            };
#pragma unroll
            for (int u = 0; u < kDispPerLane; u++)
                if (l + u * kDispLanes < ns)
                    count(clamp_sample((double)xs[u]), clamp_sample((double)ys[u]),
                          Kof(l + u * kDispLanes));
            for (int s = l + kDispResident; s < ns; s += kDispLanes) {
                const int2 i2 = ix[s];
                count(clamp_sample((double)tile[i2.x]), clamp_sample((double)em[i2.y]), Kof(s));
            }
            disp_reduce<1>(&inliers, part, tot, l);
        }
    }
    if (l == 0) {
        // abcd = (a, b, 1, d): the order D2DTransform reads (Depth.cpp:216-219, 233)
        double full[4] = {best[0], best[1], 1.0, best[2]};
        if constexpr (WEIGHTED)
            if (!(isfinite(best[0]) && isfinite(best[1]) && isfinite(best[2]))) {
                for (int i = 0; i < 4; i++) full[i] = __longlong_as_double(0x7FF8000000000000LL);
                sm.termination = kTermFailure;
            }
        const long long o = (long long)b * ntiles + p;
        for (int i = 0; i < 4; i++) {
            if (coeffs) coeffs[o * 4 + i] = (float)full[i];
            if (coeffs64) coeffs64[o * 4 + i] = full[i];
        }
        if (summary) {
            constexpr int kN = LOSS || WEIGHTED ? 6 : 4;
            summary[o * kN + 0] = sm.initial_cost;
            summary[o * kN + 1] = sm.final_cost;
            summary[o * kN + 2] = (double)sm.iterations;
            summary[o * kN + 3] = (double)sm.termination;
            if constexpr (LOSS) {
                summary[o * kN + 4] = (double)ns;
                summary[o * kN + 5] = inliers;
            }
            if constexpr (WEIGHTED) {
                summary[o * kN + 4] = used[0];
                summary[o * kN + 5] = used[1];
            }
        }
    }
}

__global__ void __launch_bounds__(kDispLanes) k_register_disp(
    const TileGeom* __restrict__ geom, const RegGrid* __restrict__ grids, int ntiles,
    const float* __restrict__ emap, long long estride, const float* __restrict__ tiles,
    long long tstride, const int2* __restrict__ sidx, float* __restrict__ coeffs,
    double* __restrict__ coeffs64, double* __restrict__ summary)
{
    __shared__ double part[kDispSums][kDispLanes];
    __shared__ double tot[kDispSums];
    register_disp_tile<false>(geom, grids, ntiles, emap, estride, tiles, tstride, sidx, coeffs,
                              coeffs64, summary, RegLoss{PF_LOSS_NONE, 0.0, 0.0, 0.0}, part, tot);
}

__global__ void __launch_bounds__(kDispLanes) k_register_disp_loss(
    const TileGeom* __restrict__ geom, const RegGrid* __restrict__ grids, int ntiles,
    const float* __restrict__ emap, long long estride, const float* __restrict__ tiles,
    long long tstride, const int2* __restrict__ sidx, float* __restrict__ coeffs,
    double* __restrict__ coeffs64, double* __restrict__ summary, RegLoss loss)
{
    __shared__ double part[kDispSums][kDispLanes];
    __shared__ double tot[kDispSums];
    register_disp_tile<true>(geom, grids, ntiles, emap, estride, tiles, tstride, sidx, coeffs,
                             coeffs64, summary, loss, part, tot);
}

__global__ void __launch_bounds__(kDispLanes) k_register_disp_planar(
    const TileGeom* __restrict__ geom, const RegGrid* __restrict__ grids, int ntiles,
    const float* __restrict__ emap, long long estride, const float* __restrict__ tiles,
    long long tstride, const int2* __restrict__ sidx, const float* __restrict__ kfs,
    float* __restrict__ coeffs, double* __restrict__ coeffs64, double* __restrict__ summary)
{
    __shared__ double part[kDispSums][kDispLanes];
    __shared__ double tot[kDispSums];
    register_disp_tile<false, true>(geom, grids, ntiles, emap, estride, tiles, tstride, sidx,
                                    coeffs, coeffs64, summary,
                                    RegLoss{PF_LOSS_NONE, 0.0, 0.0, 0.0}, part, tot, kfs);
}

__global__ void __launch_bounds__(kDispLanes) k_register_disp_planar_loss(
    const TileGeom* __restrict__ geom, const RegGrid* __restrict__ grids, int ntiles,
    const float* __restrict__ emap, long long estride, const float* __restrict__ tiles,
    long long tstride, const int2* __restrict__ sidx, const float* __restrict__ kfs,
    float* __restrict__ coeffs, double* __restrict__ coeffs64, double* __restrict__ summary,
    RegLoss loss)
{
    __shared__ double part[kDispSums][kDispLanes];
    __shared__ double tot[kDispSums];
    register_disp_tile<true, true>(geom, grids, ntiles, emap, estride, tiles, tstride, sidx,
                                   coeffs, coeffs64, summary, loss, part, tot, kfs);
}

__global__ void __launch_bounds__(kDispLanes) k_register_disp_weighted(
    const TileGeom* __restrict__ geom, const RegGrid* __restrict__ grids, int ntiles,
    const float* __restrict__ emap, long long estride, const float* __restrict__ tiles,
    long long tstride, const int2* __restrict__ sidx, const float* __restrict__ ws,
    long long wsstride, float* __restrict__ coeffs, double* __restrict__ coeffs64,
    double* __restrict__ summary)
{
    __shared__ double part[kDispSums][kDispLanes];
    __shared__ double tot[kDispSums];
    register_disp_tile<false, false, true>(geom, grids, ntiles, emap, estride, tiles, tstride,
                                           sidx, coeffs, coeffs64, summary,
                                           RegLoss{PF_LOSS_NONE, 0.0, 0.0, 0.0}, part, tot,
                                           nullptr, ws, wsstride);
}

__global__ void __launch_bounds__(kDispLanes) k_register_disp_planar_weighted(
    const TileGeom* __restrict__ geom, const RegGrid* __restrict__ grids, int ntiles,
    const float* __restrict__ emap, long long estride, const float* __restrict__ tiles,
    long long tstride, const int2* __restrict__ sidx, const float* __restrict__ kfs,
    const float* __restrict__ ws, long long wsstride, float* __restrict__ coeffs,
    double* __restrict__ coeffs64, double* __restrict__ summary)
{
    __shared__ double part[kDispSums][kDispLanes];
    __shared__ double tot[kDispSums];
    register_disp_tile<false, true, true>(geom, grids, ntiles, emap, estride, tiles, tstride, sidx,
                                          coeffs, coeffs64, summary,
                                          RegLoss{PF_LOSS_NONE, 0.0, 0.0, 0.0}, part, tot, kfs,
                                          ws, wsstride);
}

// The usable weight of every registration sample, in sample order: ws[b][soff + s] = u(w) of the
// element sample s reads when the raw tile value and the baseline value are finite, else 0.0f
// (u(w) = w for 0 < w < +inf in fp32, else 0).  Per panorama even with one weight set (wstride 0):
// the finiteness tests read the panorama's data.
__global__ void __launch_bounds__(256) k_disp_sample_weights(
    const TileGeom* __restrict__ geom, const RegGrid* __restrict__ grids,
    const float* __restrict__ emap, long long estride, const float* __restrict__ tiles,
    long long tstride, const float* __restrict__ weights, long long wstride,
    const int2* __restrict__ sidx, float* __restrict__ ws, long long wsstride)
{
    const int p = blockIdx.y, b = blockIdx.z;
    const RegGrid rg = grids[p];
    const long long off = geom[p].off;
    const float* tile = tiles + b * tstride + off;
    const float* wt = weights + b * wstride + off;
    const float* em = emap + b * estride;
    const int ns = (rg.cols + 1) * (rg.rows + 1);
    for (int s = blockIdx.x * 256 + threadIdx.x; s < ns; s += gridDim.x * 256) {
        const int2 i2 = sidx[rg.soff + s];
        const float w = wt[i2.x];
        const bool used = 0.0f < w && w < __uint_as_float(0x7F800000u) && isfinite(tile[i2.x]) &&
                          isfinite(em[i2.y]);
        ws[b * wsstride + rg.soff + s] = used ? w : 0.0f;
    }
}

// pf_tile_range_weights: the validity rule lo < v < hi (fp32; NaN fails) written as a weight set
// per panorama: 1.0f / 0.0f at channel 0, 0.0f in the other channels.
__global__ void __launch_bounds__(256) k_range_weights(const float* __restrict__ tiles,
                                                       long long npx, int c, float lo,
                                                       float hi, float* __restrict__ weights)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < npx;
         i += (long long)gridDim.x * 256) {
        const float v = tiles[i * c];
        weights[i * c] = (lo < v && v < hi) ? 1.0f : 0.0f;
        for (int ch = 1; ch < c; ch++) weights[i * c + ch] = 0.0f;
    }
}

// D2DTransform's per-pixel map (Depth.cpp:225-240).  The X clamps compare the float against the
// double constants 1e-4 and 1 - 1e-4 as Depth2DepthTransform's do: cubic_map's float thresholds
// decide identically (pf_internal.hpp).  A NaN passes every comparison and stays NaN.
__device__ __forceinline__ float disp_map(float X, float a, float b, float c, float d)
{
    if (X <= 9.99999974737875e-05f) X = (float)1e-4;
    else if (X > 0.99989998340606689f) X = (float)(1 - 1e-4);
    float Y = c / (a * X + b) + d;
    if (Y < 0) Y = 0;
    else if (Y > 1) Y = 1;
    return Y;
}

// D2DTransform on all tiles (channel 0), in place.
__global__ void __launch_bounds__(256) k_apply_disp(const TileGeom* __restrict__ geom, int ntiles,
                                                    float* __restrict__ tiles, long long tstride,
                                                    const float* __restrict__ coeffs)
{
    const int p = blockIdx.y, b = blockIdx.z;
    const TileGeom g = geom[p];
    const long long npx = (long long)g.w * g.h;
    const float4 abcd = *reinterpret_cast<const float4*>(coeffs + ((long long)b * ntiles + p) * 4);
    float* t = tiles + b * tstride + g.off;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < npx;
         i += (long long)gridDim.x * 256)
        t[i * g.c] = disp_map(t[i * g.c], abcd.x, abcd.y, abcd.z, abcd.w);
}

// D2DTransform composed with the ray factor (pf_set_tile_depth), src -> dst (in place when they
// are equal): clamp01(kf * T32(X)), T32 = disp_map's fp32 value before its final clamp, in its
// operation order; one fp32 multiply by kf; NaN stays NaN.
__global__ void __launch_bounds__(256) k_apply_disp_planar(
    const TileGeom* __restrict__ geom, const RayTile* __restrict__ ray,
    const double* __restrict__ tab, int ntiles, const float* src, float* dst, long long tstride,
    const float* __restrict__ coeffs)
{
    const int p = blockIdx.y, b = blockIdx.z;
    const TileGeom g = geom[p];
    const RayTile rt = ray[p];
    const long long npx = (long long)g.w * g.h;
    const float4 abcd = *reinterpret_cast<const float4*>(coeffs + ((long long)b * ntiles + p) * 4);
    const float* in = src + b * tstride + g.off;
    float* t = dst + b * tstride + g.off;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < npx;
         i += (long long)gridDim.x * 256) {
        float X = in[i * g.c];
        if (X <= 9.99999974737875e-05f) X = (float)1e-4;  // disp_map's clamps
        else if (X > 0.99989998340606689f) X = (float)(1 - 1e-4);
        float Y = abcd.z / (abcd.x * X + abcd.y) + abcd.w;
        Y = ray_kf(tab, rt, (int)i % g.w, (int)i / g.w) * Y;
        if (Y < 0) Y = 0;
        else if (Y > 1) Y = 1;
        t[i * g.c] = Y;
    }
}

// D2DTransform of one map, channel 0 of every pixel, in place.
__global__ void __launch_bounds__(256) k_disp_map(float* __restrict__ data, long long npx, int c,
                                                  float a, float b, float cc, float d)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < npx;
         i += (long long)gridDim.x * 256)
        data[i * c] = disp_map(data[i * c], a, b, cc, d);
}

void launch_register_disp(hipStream_t s, const TileGeom* geom, const RegGrid* grids, int ntiles,
                          const float* emap, long long estride, const float* tiles,
                          long long tstride, const int2* sidx, float* coeffs, double* coeffs64,
                          double* summary, int batch, int loss_kind, double loss_a)
{
    if (loss_kind != PF_LOSS_NONE) {
        hipLaunchKernelGGL(k_register_disp_loss, dim3((unsigned)(ntiles * batch)),
                           dim3(kDispLanes), 0, s, geom, grids, ntiles, emap, estride, tiles,
                           tstride, sidx, coeffs, coeffs64, summary,
                           make_loss(loss_kind, loss_a));
        return;
    }
    hipLaunchKernelGGL(k_register_disp, dim3((unsigned)(ntiles * batch)), dim3(kDispLanes), 0, s,
                       geom, grids, ntiles, emap, estride, tiles, tstride, sidx, coeffs, coeffs64,
                       summary);
}

void launch_register_disp_planar(hipStream_t s, const TileGeom* geom, const RegGrid* grids,
                                 int ntiles, const float* emap, long long estride,
                                 const float* tiles, long long tstride, const int2* sidx,
                                 const float* kfs, float* coeffs, double* coeffs64,
                                 double* summary, int batch, int loss_kind, double loss_a)
{
    const dim3 grid((unsigned)(ntiles * batch)), block(kDispLanes);
    if (loss_kind != PF_LOSS_NONE)
        hipLaunchKernelGGL(k_register_disp_planar_loss, grid, block, 0, s, geom, grids, ntiles,
                           emap, estride, tiles, tstride, sidx, kfs, coeffs, coeffs64, summary,
                           make_loss(loss_kind, loss_a));
    else
        hipLaunchKernelGGL(k_register_disp_planar, grid, block, 0, s, geom, grids, ntiles, emap,
                           estride, tiles, tstride, sidx, kfs, coeffs, coeffs64, summary);
}

void launch_disp_sample_weights(hipStream_t s, const TileGeom* geom, const RegGrid* grids,
                                int ntiles, int max_samples, const float* emap, long long estride,
                                const float* tiles, long long tstride, const float* weights,
                                long long wstride, const int2* sidx, float* ws, long long wsstride,
                                int batch)
{
    unsigned gx = (unsigned)((max_samples + 255) / 256);
    if (gx < 1) gx = 1;
    if (gx > 1024) gx = 1024;
    hipLaunchKernelGGL(k_disp_sample_weights, dim3(gx, (unsigned)ntiles, (unsigned)batch),
                       dim3(256), 0, s, geom, grids, emap, estride, tiles, tstride, weights,
                       wstride, sidx, ws, wsstride);
}

void launch_register_disp_weighted(hipStream_t s, const TileGeom* geom, const RegGrid* grids,
                                   int ntiles, const float* emap, long long estride,
                                   const float* tiles, long long tstride, const int2* sidx,
                                   const float* kfs, const float* ws, long long wsstride,
                                   float* coeffs, double* coeffs64, double* summary, int batch)
{
    const dim3 grid((unsigned)(ntiles * batch)), block(kDispLanes);
    if (kfs)
        hipLaunchKernelGGL(k_register_disp_planar_weighted, grid, block, 0, s, geom, grids, ntiles,
                           emap, estride, tiles, tstride, sidx, kfs, ws, wsstride, coeffs,
                           coeffs64, summary);
    else
        hipLaunchKernelGGL(k_register_disp_weighted, grid, block, 0, s, geom, grids, ntiles, emap,
                           estride, tiles, tstride, sidx, ws, wsstride, coeffs, coeffs64, summary);
}

void launch_range_weights(hipStream_t s, const float* tiles, long long npx, int c, float lo,
                          float hi, float* weights)
{
    long long gx = (npx + 255) / 256;
    if (gx > 4096) gx = 4096;
    if (gx < 1) gx = 1;
    hipLaunchKernelGGL(k_range_weights, dim3((unsigned)gx), dim3(256), 0, s, tiles, npx, c, lo,
                       hi, weights);
}

void launch_apply_disp_planar(hipStream_t s, const TileGeom* geom, const RayTile* ray,
                              const double* tab, int ntiles, long long tile_pixels,
                              const float* src, float* dst, long long tstride,
                              const float* coeffs, int batch)
{
    const long long per = tile_pixels / (ntiles > 0 ? ntiles : 1);
    long long gx = (per + 255) / 256;
    if (gx > 1024) gx = 1024;
    if (gx < 1) gx = 1;
    hipLaunchKernelGGL(k_apply_disp_planar, dim3((unsigned)gx, ntiles, batch), dim3(256), 0, s,
                       geom, ray, tab, ntiles, src, dst, tstride, coeffs);
}

void launch_apply_disp(hipStream_t s, const TileGeom* geom, int ntiles, long long tile_pixels,
                       float* tiles, long long tstride, const float* coeffs, int batch)
{
    const long long per = tile_pixels / (ntiles > 0 ? ntiles : 1);
    long long gx = (per + 255) / 256;
    if (gx > 1024) gx = 1024;
    if (gx < 1) gx = 1;
    hipLaunchKernelGGL(k_apply_disp, dim3((unsigned)gx, ntiles, batch), dim3(256), 0, s, geom, ntiles, tiles,
                       tstride, coeffs);
}

void launch_disp_map(hipStream_t s, float* data, long long npx, int c, const float* abcd)
{
    long long gx = (npx + 255) / 256;
    if (gx > 4096) gx = 4096;
    if (gx < 1) gx = 1;
    hipLaunchKernelGGL(k_disp_map, dim3((unsigned)gx), dim3(256), 0, s, data, npx, c, abcd[0], abcd[1],
                       abcd[2], abcd[3]);
}

}  // namespace pf
