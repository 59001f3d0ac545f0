// Fits the registration models on sample arrays with the reference's own Ceres 1.13 under a
// ceres::LossFunction, the way a user of the reference gets a robust registration: NULL replaced
// by new ceres::HuberLoss(a) / new ceres::SoftLOneLoss(a) at the AddResidualBlock calls
// (Depth.cpp:1232, 1393).  Compiled by tools/make_robust_golden.py against the reference's
// vendored Ceres headers and archive (never committed); builds only where the reference exists.
// The functors restate the reference's residuals (Depth.cpp:1122-1138, 1044-1073) with weight 1:
// one residual, one parameter block of size 1 per coefficient, start (1, ..., 1), DENSE_SCHUR,
// default options.
//   robust_ref_harness cubic|disparity none|huber|softl1 <a> <n> <xs.f64> <ys.f64>
//       "FIT a b c d" (disparity: a b 1 d), "COST initial final" at %.17g, "ITER <entries of
//       Summary::iterations>", "TYPE <termination_type>", "MSG <message>"
#include "ceres/ceres.h"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

struct Cubic {
    Cubic(double x, double y) : X(x), Y(y), X2(x * x), X3(x * x * x) {}
    template <typename T>
    bool operator()(const T* const a, const T* const b, const T* const c, const T* const d,
                    T* residual) const
    {
        residual[0] = T(X3) * a[0] + T(X2) * b[0] + T(X) * c[0] + d[0] - T(Y);
        return true;
    }
    double X, Y, X2, X3;
};

struct Disparity {
    Disparity(double x, double y) : X(x), Y(y) {}
    template <typename T>
    bool operator()(const T* const a, const T* const b, const T* const d, T* residual) const
    {
        residual[0] = T(1) / (a[0] * T(X) + b[0]) + d[0] - T(Y);
        return true;
    }
    double X, Y;
};

static std::vector<double> read_all(const char* fn, size_t n)
{
    std::vector<double> v(n);
    FILE* f = std::fopen(fn, "rb");
    if (!f || std::fread(v.data(), sizeof(double), n, f) != n) {
        std::fprintf(stderr, "cannot read %zu doubles of %s\n", n, fn);
        std::exit(4);
    }
    std::fclose(f);
    return v;
}

int main(int argc, char** argv)
{
    if (argc != 7) return 2;
    const std::string model(argv[1]), loss(argv[2]);
    const double a = std::atof(argv[3]);
    const size_t n = (size_t)std::atol(argv[4]);
    const std::vector<double> xs = read_all(argv[5], n), ys = read_all(argv[6], n);
    double vars[4] = {1.0, 1.0, 1.0, 1.0};
    ceres::Problem problem;
    for (size_t i = 0; i < n; i++) {
        ceres::LossFunction* lf = nullptr;  // owned by the problem
        if (loss == "huber") lf = new ceres::HuberLoss(a);
        else if (loss == "softl1") lf = new ceres::SoftLOneLoss(a);
        else if (loss != "none") return 2;
        if (model == "cubic")
            problem.AddResidualBlock(
                new ceres::AutoDiffCostFunction<Cubic, 1, 1, 1, 1, 1>(new Cubic(xs[i], ys[i])), lf,
                &vars[0], &vars[1], &vars[2], &vars[3]);
        else if (model == "disparity")
            problem.AddResidualBlock(
                new ceres::AutoDiffCostFunction<Disparity, 1, 1, 1, 1>(new Disparity(xs[i], ys[i])),
                lf, &vars[0], &vars[1], &vars[3]);
        else
            return 2;
    }
    ceres::Solver::Options options;
    options.linear_solver_type = ceres::DENSE_SCHUR;
    ceres::Solver::Summary summary;
    ceres::Solve(options, &problem, &summary);
    if (model == "disparity") vars[2] = 1.0;
    std::printf("FIT %.17g %.17g %.17g %.17g\n", vars[0], vars[1], vars[2], vars[3]);
    std::printf("COST %.17g %.17g\n", summary.initial_cost, summary.final_cost);
    std::printf("ITER %d\n", (int)summary.iterations.size());
    std::printf("TYPE %d\n", (int)summary.termination_type);
    std::printf("MSG %s\n", summary.message.c_str());
    return 0;
}
