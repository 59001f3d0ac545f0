"""CPU restatement of the device solver lm_solve (csrc/pf_lm.hpp): the Ceres 1.13 trust-region
Levenberg-Marquardt (DENSE_SCHUR, default options, the first parameter eliminated) that the
registration fits share.  disp_ref.fit, robust_ref.fit and global_ref.lm_moments call it.

TEST INFRASTRUCTURE ONLY.  The scalar algebra runs on Python floats, operation for operation as
the device code: every operation is an IEEE-754 fp64 + - * / or sqrt, correctly rounded on both
sides, so the two agree bit for bit.
"""
import math

import numpy as np

MAX_ITER = 50
INIT_RADIUS, MAX_RADIUS, MIN_RADIUS = 1e4, 1e16, 1e-32
MIN_REL_DECREASE, MIN_DIAG, MAX_DIAG = 1e-3, 1e-6, 1e32
MAX_INVALID = 5
FUNC_TOL, GRAD_TOL, PARAM_TOL = 1e-6, 1e-10, 1e-8
DBL_MAX = float(np.finfo(np.float64).max)
TERMINATION = ("no_convergence", "function_tolerance", "parameter_tolerance",
               "gradient_tolerance", "min_trust_region_radius", "failure")


def _sqrt(v):
    return math.sqrt(v) if v >= 0.0 else float("nan")


def _inv_psd1(v):
    l = math.sqrt(v)
    return (1.0 / l) / l


def _llt_solve(S, rhs):
    """Eigen LLT<Upper> of the reduced Schur system and its two triangular solves (llt_solve)."""
    n = len(rhs)
    L = [[0.0] * n for _ in range(n)]
    for k in range(n):
        x = S[k][k]
        if k > 0:
            sq = 0.0
            for i in range(k):
                sq = sq + L[k][i] * L[k][i]
            x = x - sq
        if not x > 0.0:
            return None
        x = math.sqrt(x)
        L[k][k] = x
        for j in range(k + 1, n):
            v = S[k][j]
            for i in range(k):
                v = v - L[j][i] * L[k][i]
            L[j][k] = v / x
    y = list(rhs)
    for k in range(n):
        y[k] = y[k] / L[k][k]
        for j in range(k + 1, n):
            y[j] = y[j] - L[j][k] * y[k]
    for k in range(n - 1, -1, -1):
        y[k] = y[k] / L[k][k]
        for j in range(k):
            y[j] = y[j] - L[k][j] * y[k]
    return y


def _norm(v):
    s = v[0] * v[0]
    for k in range(1, len(v)):
        s = s + v[k] * v[k]
    return math.sqrt(s)


def solve(start, evaluate, trial, non_finite_trial_invalid, trace=None):
    """The fit from `start`.  evaluate(x) -> (cost, g, M): the cost, the gradient J'r and the
    unscaled J'J at x; trial(x) -> a trial cost.

    non_finite_trial_invalid is lm_solve's switch.  False (the moment form): the trial is evaluated
    for every valid step, after the run of invalid steps is reset, and a cost that is not finite
    becomes DBL_MAX.  True (the sample-wise kernels): a trial whose cost is not finite makes the
    step invalid and counts into that run.

    Returns (best, summary dict).  trace (optional list) receives one dict per iteration:
    iteration, the radius, parameters x and cost it started from, and the outcome of its step.
    """
    n = len(start)
    m = n - 1
    x = [float(v) for v in start]
    best = list(x)
    x_cost, g, M = evaluate(x)
    sc = [1.0 / (1.0 + _sqrt(M[k][k])) for k in range(n)]

    def scale(M):
        return [[(M[i][j] * sc[i]) * sc[j] for j in range(n)] for i in range(n)]

    Ms = scale(M)
    initial_cost = x_cost
    radius, decrease, x_norm, min_cost = INIT_RADIUS, 2.0, -1.0, DBL_MAX
    reuse_diag, successful = False, True
    invalid_run, iteration, term = 0, 0, 0
    diag = [0.0] * n
    while True:
        if successful and x_cost < min_cost:
            min_cost = x_cost
            best = list(x)
        if iteration >= MAX_ITER:
            term = 0
            break
        if successful:
            gmax = 0.0
            for k in range(n):
                d = abs(x[k] - (x[k] + -g[k]))
                if d > gmax:
                    gmax = d
            if gmax <= GRAD_TOL:
                term = 3
                break
        if radius <= MIN_RADIUS:
            term = 4
            break
        iteration += 1
        rec = {"iteration": iteration, "radius": radius, "x": tuple(x), "cost": x_cost,
               "outcome": None}
        if trace is not None:
            trace.append(rec)
        if not reuse_diag:
            for k in range(n):
                d = Ms[k][k] if Ms[k][k] > MIN_DIAG else MIN_DIAG
                diag[k] = d if d < MAX_DIAG else MAX_DIAG
        D = [math.sqrt(diag[k] / radius) for k in range(n)]
        gs = [sc[k] * g[k] for k in range(n)]
        ete = D[0] * D[0] + Ms[0][0]
        R = [[0.0] * m for _ in range(m)]
        for a in range(m):
            for c in range(a, m):
                R[a][c] = Ms[1 + a][1 + c] + (D[1 + a] * D[1 + a] if a == c else 0.0)
        inv = _inv_psd1(ete)
        inv_g = inv * gs[0]
        rhs = [gs[1 + a] - Ms[0][1 + a] * inv_g for a in range(m)]
        for a in range(m):
            bt = Ms[0][1 + a] * inv
            for c in range(a, m):
                R[a][c] = R[a][c] - bt * Ms[0][1 + c]
        z = _llt_solve(R, rhs)
        ok = z is not None
        step = [0.0] * n
        if ok:
            ya = gs[0]
            for a in range(m):
                ya = ya - Ms[0][1 + a] * z[a]
            step = [inv * ya] + list(z)
            ok = all(math.isfinite(v) for v in step)
        reuse_diag = True
        mcc, cand_cost, valid = 0.0, 0.0, False
        if ok:
            step = [v * -1.0 for v in step]
            sJr, sMs = 0.0, 0.0
            for i in range(n):
                q = 0.0
                for j in range(n):
                    q = q + Ms[i][j] * step[j]
                sMs = sMs + step[i] * q
                sJr = sJr + step[i] * gs[i]
            mcc = -(sJr + sMs / 2.0)
            valid = mcc > 0.0
        if non_finite_trial_invalid and valid:
            cand = [x[k] + step[k] * sc[k] for k in range(n)]
            cand_cost = trial(cand)
            valid = math.isfinite(cand_cost)  # a failed evaluation: an invalid step
        if not valid:
            rec["outcome"] = "invalid"
            invalid_run += 1
            if invalid_run >= MAX_INVALID:
                term = 5
                break
            radius = radius / decrease
            decrease *= 2.0
            successful = False
            continue
        invalid_run = 0
        if not non_finite_trial_invalid:
            cand = [x[k] + step[k] * sc[k] for k in range(n)]
            cand_cost = trial(cand)
            if not math.isfinite(cand_cost):
                cand_cost = DBL_MAX
        dx = [x[k] - cand[k] for k in range(n)]
        if _norm(dx) <= PARAM_TOL * (x_norm + PARAM_TOL):
            rec["outcome"] = "parameter_tolerance"
            term = 2
            break
        if abs(x_cost - cand_cost) <= FUNC_TOL * x_cost:
            rec["outcome"] = "function_tolerance"
            term = 1
            break
        rel = (x_cost - cand_cost) / mcc
        if rel > MIN_REL_DECREASE:
            rec["outcome"] = "accepted"
            x = list(cand)
            x_norm = _norm(x)
            x_cost, g, M = evaluate(x)
            Ms = scale(M)
            q = 2.0 * rel - 1.0
            f = 1.0 - q * q * q
            radius = radius / (f if f > 1.0 / 3.0 else 1.0 / 3.0)
            radius = radius if radius < MAX_RADIUS else MAX_RADIUS
            decrease = 2.0
            reuse_diag = False
            successful = True
        else:
            rec["outcome"] = "rejected"
            radius = radius / decrease
            decrease *= 2.0
            successful = False
    summary = {"initial_cost": initial_cost, "final_cost": min_cost, "iterations": iteration,
               "termination": TERMINATION[term], "termination_code": term,
               "final_radius": radius, "x": tuple(x)}
    return best, summary


def unpack_sums(S, n):
    """(cost, g, M) from the sums of a sample-wise Jacobian evaluation: the cost, the n of J'r,
    the n (n + 1) / 2 of upper J'J row by row."""
    M = [[0.0] * n for _ in range(n)]
    at = 1 + n
    for i in range(n):
        for j in range(i, n):
            M[i][j] = M[j][i] = S[at]
            at += 1
    return S[0], [S[1 + i] for i in range(n)], M
