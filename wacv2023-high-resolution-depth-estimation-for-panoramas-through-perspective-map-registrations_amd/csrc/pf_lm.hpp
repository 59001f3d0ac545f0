// pf_lm.hpp -- what the registration solvers share (pf_register.hip, pf_disp.hip, pf_robust.hip):
// the Ceres 1.13 trust-region Levenberg-Marquardt driver lm_solve with its constants and small
// dense helpers, the sample clamp, the 256-lane ordered reduction and the robust loss functions of
// pf_set_register_loss.  Device code only; fp64 + - * / sqrt, no contraction.
#pragma once
#include "pf_internal.hpp"

#include <cfloat>

namespace pf {

constexpr int kDispLanes = 256;
// Resident capacity: samples of one tile kept in registers across the LM iterations
// (kDispPerLane (X, Y) pairs per lane, as the floats they were read as: the clamp to fp64 is
// repeated per use).  Samples past it are gathered again from the cached indices in every
// evaluation, in the same per-lane order.
constexpr int kDispPerLane = 32;
constexpr int kDispResident = kDispLanes * kDispPerLane;

constexpr int kLmMaxIter = 50;
constexpr double kLmInitRadius = 1e4, kLmMaxRadius = 1e16, kLmMinRadius = 1e-32;
constexpr double kLmMinRelDecrease = 1e-3, kLmMinDiag = 1e-6, kLmMaxDiag = 1e32;
constexpr int kLmMaxInvalid = 5;
constexpr double kLmFuncTol = 1e-6, kLmGradTol = 1e-10, kLmParamTol = 1e-8;
// termination codes of the summary (the order of pfo_lm_summary's)
enum { kTermNoConvergence = 0, kTermFunctionTol, kTermParameterTol, kTermGradientTol,
       kTermMinRadius, kTermFailure };

__device__ __forceinline__ double clamp_sample(double v)
{  // Depth.cpp:1352-1362
    if (v < 1e-4) v = 1e-4;
    else if (v > (1 - 1e-4)) v = 1 - 1e-4;
    return v;
}

// The ray factor of pixel (i, j) of a planar-depth tile (pf_set_tile_depth) from the layout's
// column / row tables (pf_ray.hpp): two fp64 adds and an fp64 sqrt, rounded once to fp32 -- the one
// definition of kf.
__device__ __forceinline__ float ray_kf(const double* __restrict__ tab, const RayTile rt, int i,
                                        int j)
{
    return (float)sqrt(1.0 + tab[rt.cu + i] + tab[rt.rv + j]);
}

// The halving tree over the 256 lanes' partial sums, every lane receiving the totals.  Strides
// 128 and 64 are wave 0 reading the four waves' values from LDS, strides 32..1 its lane shifts:
// the same additions in the same association as p[l] = p[l] + p[l + stride].
template <int N>
__device__ __forceinline__ void disp_reduce(double* acc, double (*part)[kDispLanes], double* tot,
                                            int l)
{
#pragma unroll
    for (int k = 0; k < N; k++) part[k][l] = acc[k];
    __syncthreads();
    if (l < 64) {
#pragma unroll
        for (int k = 0; k < N; k++) {
            double v = (part[k][l] + part[k][l + 128]) + (part[k][l + 64] + part[k][l + 192]);
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) v = v + __shfl_down(v, s, 64);
            if (l == 0) tot[k] = v;
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; k++) acc[k] = tot[k];
}

// ---------------------------------------------------------------------------------------------
// The reference's registration solver: Ceres 1.13 trust-region Levenberg-Marquardt, DENSE_SCHUR,
// default options, the first parameter eliminated.  Every rule (Jacobi column scaling, LM diagonal
// and radius updates, step validity and quality, the parameter/function/gradient tolerances,
// returning the best accepted point) is cited in oracle/pf_oracle_lm.c, whose pfo_lm_moments is
// this loop operation for operation on the moment form, so the two agree bit for bit.
struct LmSummary {
    double initial_cost, final_cost;  // final: the minimum over the accepted points
    int iterations, termination;      // kTerm*
};

__device__ __forceinline__ double inv_psd1(double v)
{  // Eigen LLT of a 1x1 block solved against 1 (InvertPSDMatrix, full rank)
    const double l = sqrt(v);
    return (1.0 / l) / l;
}

template <int N>
__device__ bool llt_solve(const double (&S)[N][N], const double (&rhs)[N], double (&z)[N])
{  // Eigen LLT<Upper> of the reduced Schur system (schur_complement_solver.cc:197-213)
    double L[N][N];
    for (int i = 0; i < N; i++)
        for (int j = 0; j < N; j++) L[i][j] = 0.0;
    for (int k = 0; k < N; k++) {
        double x = S[k][k];
        if (k > 0) {
            double sq = 0.0;
            for (int i = 0; i < k; i++) sq = sq + L[k][i] * L[k][i];
            x = x - sq;
        }
        if (!(x > 0.0)) return false;
        L[k][k] = x = sqrt(x);
        for (int j = k + 1; j < N; j++) {
            double a = S[k][j];
            for (int i = 0; i < k; i++) a = a - L[j][i] * L[k][i];
            L[j][k] = a / x;
        }
    }
    double y[N];
    for (int k = 0; k < N; k++) y[k] = rhs[k];
    for (int k = 0; k < N; k++) {
        y[k] = y[k] / L[k][k];
        for (int j = k + 1; j < N; j++) y[j] = y[j] - L[j][k] * y[k];
    }
    for (int k = N - 1; k >= 0; k--) {
        y[k] = y[k] / L[k][k];
        for (int j = 0; j < k; j++) y[j] = y[j] - L[k][j] * y[k];
    }
    for (int k = 0; k < N; k++) z[k] = y[k];
    return true;
}

template <int N>
__device__ __forceinline__ double norm(const double (&v)[N])
{  // left-associated
    double s = v[0] * v[0];
    for (int k = 1; k < N; k++) s = s + v[k] * v[k];
    return sqrt(s);
}

// The fit of N parameters from `start`.  eval_full(x, cost, g, M) returns the cost, the gradient
// J'r and the unscaled J'J at x; eval_cost(x) returns a trial cost.  best receives the accepted
// point of least cost.
//
// kNonFiniteTrialInvalid is the one place where the solvers differ.  false (the moment form,
// lm_moments, as pfo_lm_moments): the trial is evaluated for every valid step, after the run of
// invalid steps is reset, and a cost that is not finite becomes DBL_MAX.  true (the sample-wise
// kernels): a trial whose cost is not finite is a failed evaluation, so the step is invalid and
// counts into that run.
//
// The callers of the sample-wise kernels run this on every lane of a block with the same reduced
// sums, hence the same state: all exits are block-uniform, and eval_full / eval_cost may hold
// block barriers.  Those kernels sit at the VGPR limit: the trial evaluation
// is written out at its two places because a local lambda around it cost k_register_robust its
// second wave per SIMD.
template <int N, bool kNonFiniteTrialInvalid, class EvalFull, class EvalCost>
__device__ __forceinline__ void lm_solve(const double (&start)[N], EvalFull&& eval_full,
                                         EvalCost&& eval_cost, double (&best)[N], LmSummary& out)
{
    double x[N], sc[N], M[N][N], Ms[N][N], g[N], gs[N], diag[N], D[N], step[N], cand[N];
    for (int k = 0; k < N; k++) {
        x[k] = best[k] = start[k];
        diag[k] = 0.0;
    }
    auto scale = [&]() {  // the scaled J'J of a Jacobian evaluation
        for (int i = 0; i < N; i++)
            for (int j = 0; j < N; j++) Ms[i][j] = (M[i][j] * sc[i]) * sc[j];
    };
    double x_cost;
    eval_full(x, x_cost, g, M);
    for (int k = 0; k < N; k++) sc[k] = 1.0 / (1.0 + sqrt(M[k][k]));  // Jacobi scaling, fixed here
    scale();
    const double initial_cost = x_cost;
    double radius = kLmInitRadius, decrease = 2.0, x_norm = -1.0, min_cost = DBL_MAX;
    bool reuse_diag = false, successful = true;
    int invalid_run = 0, iteration = 0, term = kTermNoConvergence;
    for (;;) {
        if (successful && x_cost < min_cost) {
            min_cost = x_cost;
            for (int k = 0; k < N; k++) best[k] = x[k];
        }
        if (iteration >= kLmMaxIter) { term = kTermNoConvergence; break; }
        if (successful) {
            double gmax = 0.0;
            for (int k = 0; k < N; k++) {
                const double d = fabs(x[k] - (x[k] + -g[k]));
                if (d > gmax) gmax = d;
            }
            if (gmax <= kLmGradTol) { term = kTermGradientTol; break; }
        }
        if (radius <= kLmMinRadius) { term = kTermMinRadius; break; }
        iteration++;
        if (!reuse_diag)
            for (int k = 0; k < N; k++) {
                const double d = Ms[k][k] > kLmMinDiag ? Ms[k][k] : kLmMinDiag;
                diag[k] = d < kLmMaxDiag ? d : kLmMaxDiag;
            }
        for (int k = 0; k < N; k++) D[k] = sqrt(diag[k] / radius);
        for (int k = 0; k < N; k++) gs[k] = sc[k] * g[k];
        const double ete = D[0] * D[0] + Ms[0][0];
        double R[N - 1][N - 1], rhs[N - 1], z[N - 1];
        for (int a = 0; a < N - 1; a++)
            for (int c = a; c < N - 1; c++)
                R[a][c] = Ms[1 + a][1 + c] + (a == c ? D[1 + a] * D[1 + a] : 0.0);
        const double inv = inv_psd1(ete);
        const double inv_g = inv * gs[0];
        for (int a = 0; a < N - 1; a++) rhs[a] = gs[1 + a] - Ms[0][1 + a] * inv_g;
        for (int a = 0; a < N - 1; a++) {
            const double bt = Ms[0][1 + a] * inv;
            for (int c = a; c < N - 1; c++) R[a][c] = R[a][c] - bt * Ms[0][1 + c];
        }
        bool ok = llt_solve(R, rhs, z);
        if (ok) {
            double ya = gs[0];
            for (int a = 0; a < N - 1; a++) ya = ya - Ms[0][1 + a] * z[a];
            step[0] = inv * ya;
            for (int a = 0; a < N - 1; a++) step[1 + a] = z[a];
            for (int k = 0; ok && k < N; k++) ok = isfinite(step[k]);
        }
        reuse_diag = true;
        double mcc = 0.0, cand_cost = 0.0;
        bool valid = false;
        if (ok) {
            for (int k = 0; k < N; k++) step[k] = step[k] * -1.0;
            double sJr = 0.0, sMs = 0.0;
            for (int i = 0; i < N; i++) {
                double q = 0.0;
                for (int j = 0; j < N; j++) q = q + Ms[i][j] * step[j];
                sMs = sMs + step[i] * q;
                sJr = sJr + step[i] * gs[i];
            }
            mcc = -(sJr + sMs / 2.0);
            valid = mcc > 0.0;
        }
        if constexpr (kNonFiniteTrialInvalid)
            if (valid) {
                for (int k = 0; k < N; k++) cand[k] = x[k] + step[k] * sc[k];
                cand_cost = eval_cost(cand);
                valid = isfinite(cand_cost);
            }
        if (!valid) {
            if (++invalid_run >= kLmMaxInvalid) { term = kTermFailure; break; }
            radius = radius / decrease;
            decrease *= 2.0;
            successful = false;
            continue;
        }
        invalid_run = 0;
        if constexpr (!kNonFiniteTrialInvalid) {
            for (int k = 0; k < N; k++) cand[k] = x[k] + step[k] * sc[k];
            cand_cost = eval_cost(cand);
            if (!isfinite(cand_cost)) cand_cost = DBL_MAX;
        }
        double dx[N];
        for (int k = 0; k < N; k++) dx[k] = x[k] - cand[k];
        if (norm(dx) <= kLmParamTol * (x_norm + kLmParamTol)) { term = kTermParameterTol; break; }
        if (fabs(x_cost - cand_cost) <= kLmFuncTol * x_cost) { term = kTermFunctionTol; break; }
        const double rel = (x_cost - cand_cost) / mcc;
        if (rel > kLmMinRelDecrease) {
            for (int k = 0; k < N; k++) x[k] = cand[k];
            x_norm = norm(x);
            eval_full(x, x_cost, g, M);
            scale();
            const double q = 2.0 * rel - 1.0;
            const double f = 1.0 - q * q * q;
            radius = radius / (f > 1.0 / 3.0 ? f : 1.0 / 3.0);
            radius = radius < kLmMaxRadius ? radius : kLmMaxRadius;
            decrease = 2.0;
            reuse_diag = false;
            successful = true;
        } else {
            radius = radius / decrease;
            decrease *= 2.0;
            successful = false;
        }
    }
    out.initial_cost = initial_cost;
    out.final_cost = min_cost;
    out.iterations = iteration;
    out.termination = term;
}

// A robust loss of pf_set_register_loss: kind PF_LOSS_HUBER or PF_LOSS_SOFTL1, scale a, b = a a,
// c = 1 / b (Ceres 1.13 loss_function.h:177-207).
struct RegLoss {
    int kind;
    double a, b, c;
};

__host__ __device__ inline RegLoss make_loss(int kind, double a)
{
    const double b = a * a;
    return RegLoss{kind, a, b, 1.0 / b};
}

// rho(s) and rho'(s) at the squared residual s (loss_function.cc:47-70).  rho'' <= 0 for both
// losses, so Corrector (corrector.cc:81-85) scales the residual and the Jacobian row by
// sqrt(rho') and nothing else.
__device__ __forceinline__ void loss_eval(const RegLoss& L, double s, double& rho0, double& rho1)
{
    if (L.kind == PF_LOSS_HUBER) {
        if (s > L.b) {
            const double r = sqrt(s);
            const double d = L.a / r;
            rho0 = (2.0 * L.a) * r - L.b;
            rho1 = d > DBL_MIN ? d : DBL_MIN;
        } else {
            rho0 = s;
            rho1 = 1.0;
        }
    } else {  // PF_LOSS_SOFTL1
        const double sum = 1.0 + s * L.c;
        const double tmp = sqrt(sum);
        const double d = 1.0 / tmp;
        rho0 = (2.0 * L.b) * (tmp - 1.0);
        rho1 = d > DBL_MIN ? d : DBL_MIN;
    }
}

}  // namespace pf
