// pf_lm.hpp -- what the sample-wise registration kernels share (pf_disp.hip, pf_robust.hip): the
// Ceres 1.13 trust-region constants, the sample clamp, the 256-lane ordered reduction and the
// robust loss functions of pf_set_register_loss.  Device code only; fp64 + - * / sqrt, no
// contraction.
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
{  // Depth.cpp:1352-1362, as k_register
    if (v < 1e-4) v = 1e-4;
    else if (v > (1 - 1e-4)) v = 1 - 1e-4;
    return v;
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

__device__ __forceinline__ double inv_psd1(double v)
{  // Eigen LLT of a 1x1 block solved against 1 (InvertPSDMatrix, full rank)
    const double l = sqrt(v);
    return (1.0 / l) / l;
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
