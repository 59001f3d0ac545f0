"""CPU restatement of the robust tile registration (csrc/pf_robust.hip, and the loss instantiation
of csrc/pf_disp.hip): the sample-wise Ceres 1.13 trust-region LM of the cubic
y = a x^3 + b x^2 + c x + d, or of y = 1/(a x + b) + d, under HuberLoss or SoftLOneLoss.

TEST INFRASTRUCTURE ONLY.  The fit follows the kernels operation for operation: every sum is taken
by disp_ref.ordered_sum (lane l of 256 adds samples l, l + 256, ... in order from 0.0, then the
halving tree) over elementwise numpy fp64 terms, and the scalar LM algebra runs on Python floats.
Every operation is an IEEE-754 fp64 + - * / or sqrt, correctly rounded on both sides, so the two
agree bit for bit.

Loss semantics (Ceres 1.13), with s = r r of the unscaled residual and b = a a:
  huber   (loss_function.cc:47-61)  s > b: rho = 2 a sqrt(s) - b, rho' = max(DBL_MIN, a / sqrt(s));
                                    else rho = s, rho' = 1
  softl1  (loss_function.cc:63-70)  t = sqrt(1 + s / b as s * (1 / b)): rho = 2 b (t - 1),
                                    rho' = max(DBL_MIN, 1 / t)
rho'' <= 0, so Corrector (corrector.cc:81-85) scales the residual and the Jacobian row by
sqrt(rho'); the cost term is 0.5 rho (residual_block.cc:164-166).

Under the validity rule a skipped sample keeps its lane and adds 0.0.  (The kernel adds nothing
instead; the two differ only in the sign of a partial sum that is exactly -0.0, which needs a
product that is exactly -0.0 and never changes a value.)
"""
import math

import numpy as np

import disp_ref as DR
from disp_ref import (DBL_MAX, FUNC_TOL, GRAD_TOL, INIT_RADIUS, MAX_DIAG, MAX_INVALID, MAX_ITER,
                      MAX_RADIUS, MIN_DIAG, MIN_RADIUS, MIN_REL_DECREASE, PARAM_TOL, TERMINATION)

DBL_MIN = float(np.finfo(np.float64).tiny)
LOSS_KINDS = (None, "huber", "softl1")
MODELS = {"cubic": 4, "disparity": 3}


def loss(kind, a, s):
    """(rho, rho') of the squared residuals s (fp64 array); kind None: (s, 1)."""
    s = np.asarray(s, np.float64)
    if kind is None:
        return s.copy(), np.ones_like(s)
    b = a * a
    with np.errstate(all="ignore"):
        if kind == "huber":
            r = np.sqrt(s)
            d = a / r
            big = s > b
            rho0 = np.where(big, (2.0 * a) * r - b, s)
            rho1 = np.where(big, np.where(d > DBL_MIN, d, DBL_MIN), 1.0)
            return rho0, rho1
        if kind == "softl1":
            c = 1.0 / b
            tmp = np.sqrt(1.0 + s * c)
            d = 1.0 / tmp
            return (2.0 * b) * (tmp - 1.0), np.where(d > DBL_MIN, d, DBL_MIN)
    raise ValueError(kind)


def residual_and_rows(xs, ys, p, model):
    """The unscaled residual and the Jacobian row's columns (a list of arrays or of the float 1.0)."""
    if model == "cubic":
        X2 = xs * xs
        X3 = xs * xs * xs
        r = (((X3 * p[0] + X2 * p[1]) + xs * p[2]) + p[3]) - ys
        return r, [X3, X2, xs, 1.0]
    q = 1.0 / (p[0] * xs + p[1])
    r = (q + p[2]) - ys
    qq = q * q
    return r, [-(xs * qq), -qq, 1.0]


def term_arrays(xs, ys, p, kind, a, model):
    """The per-sample terms of a Jacobian evaluation in the kernel's order: the cost term, the n of
    J'r, the n (n + 1) / 2 of upper J'J row by row (15 for the cubic, 10 for the disparity model)."""
    with np.errstate(all="ignore"):
        r, J = residual_and_rows(xs, ys, p, model)
        rho0, rho1 = loss(kind, a, r * r)
        w = np.sqrt(rho1)
        rc = w * r
        K = [w * j if not isinstance(j, float) else w for j in J]  # w * 1.0 is w
        n = len(K)
        terms = [0.5 * rho0] + [K[i] * rc for i in range(n)]
        terms += [K[i] * K[j] for i in range(n) for j in range(i, n)]
        return terms


def _masked(t, valid):
    return t if valid is None else np.where(valid, t, 0.0)


def sums(xs, ys, p, kind, a, model, valid=None, ordered_sum=None):
    ordered_sum = ordered_sum or DR.ordered_sum
    return [ordered_sum(_masked(t, valid)) for t in term_arrays(xs, ys, p, kind, a, model)]


def cost(xs, ys, p, kind, a, model, valid=None, ordered_sum=None):
    """A trial evaluation: the one sum of 0.5 rho."""
    ordered_sum = ordered_sum or DR.ordered_sum
    with np.errstate(all="ignore"):
        r, _ = residual_and_rows(xs, ys, p, model)
        rho0, _ = loss(kind, a, r * r)
        return ordered_sum(_masked(0.5 * rho0, valid))


def _inv_psd1(v):
    l = math.sqrt(v)
    return (1.0 / l) / l


def _llt_solve(S, rhs):
    """Eigen LLT<Upper> of the reduced Schur system and its two triangular solves: llt3_solve's
    loops for any size (llt2_solve is the same operations for n = 2)."""
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


def fit(xs, ys, kind, a=0.0, model="cubic", valid=None, trace=None, ordered_sum=None):
    """The LM fit on already clamped samples under the loss (kind None: plain least squares in the
    same sample-wise form).  valid: bool [ns] or None, the samples the validity rule keeps.
    Returns (coef64[4], summary dict); the disparity model's coefficients are (a, b, 1, d).
    trace (optional list) receives (iteration, cost at its start, outcome) per iteration."""
    xs = np.ascontiguousarray(xs, np.float64)
    ys = np.ascontiguousarray(ys, np.float64)
    n = MODELS[model]
    used = int(xs.size if valid is None else np.count_nonzero(valid))
    if valid is not None:
        valid = np.asarray(valid, bool)
        # a skipped sample's values never reach the arithmetic
        xs = np.where(valid, xs, 0.5)
        ys = np.where(valid, ys, 0.5)
    nan4 = np.full(4, np.nan)
    if valid is not None and used < 4:
        return nan4, {"initial_cost": math.nan, "final_cost": math.nan, "iterations": 0,
                      "termination_code": 5, "termination": TERMINATION[5], "used": used,
                      "inliers": 0}
    diag_at = []  # index of M[k][k] among the sums
    at = 1 + n
    for i in range(n):
        diag_at.append(at)
        at += n - i

    def take(S):
        M = [[0.0] * n for _ in range(n)]
        at = 1 + n
        for i in range(n):
            for j in range(i, n):
                M[i][j] = M[j][i] = S[at]
                at += 1
        g = [S[1 + i] for i in range(n)]
        Ms = [[(M[i][j] * sc[i]) * sc[j] for j in range(n)] for i in range(n)]
        return g, Ms

    x = [1.0] * n
    best = [1.0] * n
    S = sums(xs, ys, x, kind, a, model, valid, ordered_sum)
    sc = [1.0 / (1.0 + math.sqrt(S[k])) for k in diag_at]
    g, Ms = take(S)
    x_cost = S[0]
    initial_cost = x_cost
    radius, decrease, x_norm, min_cost = INIT_RADIUS, 2.0, -1.0, DBL_MAX
    reuse_diag, successful = False, True
    invalid_run, iteration, term = 0, 0, 0
    diag = [0.0] * n
    m = n - 1
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
        rec = [iteration, x_cost, None]
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
        for i in range(m):
            for c in range(i, m):
                R[i][c] = Ms[1 + i][1 + c] + (D[1 + i] * D[1 + i] if i == c else 0.0)
        inv = _inv_psd1(ete)
        inv_g = inv * gs[0]
        rhs = [gs[1 + i] - Ms[0][1 + i] * inv_g for i in range(m)]
        for i in range(m):
            bt = Ms[0][1 + i] * inv
            for c in range(i, m):
                R[i][c] = R[i][c] - bt * Ms[0][1 + c]
        z = _llt_solve(R, rhs)
        ok = z is not None
        step = [0.0] * n
        if ok:
            ya = gs[0]
            for i in range(m):
                ya = ya - Ms[0][1 + i] * z[i]
            step = [inv * ya] + list(z)
            ok = all(math.isfinite(v) for v in step)
        reuse_diag = True
        mcc, cand_cost, ok_step = 0.0, 0.0, False
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
            ok_step = mcc > 0.0
        if ok_step:
            cand = [x[k] + step[k] * sc[k] for k in range(n)]
            cand_cost = cost(xs, ys, cand, kind, a, model, valid, ordered_sum)
            ok_step = math.isfinite(cand_cost)  # a failed evaluation: an invalid step
        if not ok_step:
            rec[2] = "invalid"
            invalid_run += 1
            if invalid_run >= MAX_INVALID:
                term = 5
                break
            radius = radius / decrease
            decrease *= 2.0
            successful = False
            continue
        invalid_run = 0
        dx = [x[k] - cand[k] for k in range(n)]
        if _norm(dx) <= PARAM_TOL * (x_norm + PARAM_TOL):
            rec[2] = "parameter_tolerance"
            term = 2
            break
        if abs(x_cost - cand_cost) <= FUNC_TOL * x_cost:
            rec[2] = "function_tolerance"
            term = 1
            break
        rel = (x_cost - cand_cost) / mcc
        if rel > MIN_REL_DECREASE:
            rec[2] = "accepted"
            x = list(cand)
            x_norm = _norm(x)
            S = sums(xs, ys, x, kind, a, model, valid, ordered_sum)
            g, Ms = take(S)
            x_cost = S[0]
            q = 2.0 * rel - 1.0
            f = 1.0 - q * q * q
            radius = radius / (f if f > 1.0 / 3.0 else 1.0 / 3.0)
            radius = radius if radius < MAX_RADIUS else MAX_RADIUS
            decrease = 2.0
            reuse_diag = False
            successful = True
        else:
            rec[2] = "rejected"
            radius = radius / decrease
            decrease *= 2.0
            successful = False
    with np.errstate(all="ignore"):
        r, _ = residual_and_rows(xs, ys, best, model)
        inl = (r * r) <= a * a
        if valid is not None:
            inl = inl & valid
    if model == "cubic":
        coef = np.array(best, np.float64)
        if not all(math.isfinite(v) for v in best):  # k_register_robust's guard
            coef, term = nan4, 5
    else:
        coef = np.array([best[0], best[1], 1.0, best[2]], np.float64)
    summary = {"initial_cost": initial_cost, "final_cost": min_cost, "iterations": iteration,
               "termination": TERMINATION[term], "termination_code": term, "used": used,
               "inliers": int(np.count_nonzero(inl))}
    return coef, summary


def summary_row(summary):
    """The kernel's per-tile summary: 6 doubles."""
    return np.array([summary["initial_cost"], summary["final_cost"],
                     float(summary["iterations"]), float(summary["termination_code"]),
                     float(summary["used"]), float(summary["inliers"])], np.float64)


def cubic(c, x):
    """The fitted cubic at x, fp64."""
    x = np.asarray(x, np.float64)
    return ((c[0] * x ** 3 + c[1] * x ** 2) + c[2] * x) + c[3]


# ---- planted outliers --------------------------------------------------------------------------
OUTLIER_SEEDS = (0, 1, 2, 3, 4)
OUTLIER_N = 2409
GRID = np.linspace(0.1, 0.6, 101)


def truth(x):
    return 0.9 * np.asarray(x, np.float64) ** 1.1 + 0.02


def planted_samples(seed, n=OUTLIER_N, frac=0.10):
    """n samples of the truth over x in 0.1-0.6 with noise sigma 0.002, a fraction of the y values
    replaced by U(0, 1); clamped as the registration clamps.  Returns (xs, ys, outlier mask)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.1, 0.6, n)
    y = truth(x) + rng.normal(0, 0.002, n)
    out = rng.random(n) < frac
    y[out] = rng.uniform(0, 1, int(out.sum()))
    return DR.clamp_samples(x), DR.clamp_samples(y), out


def max_error(c):
    """max |fit - truth| over x in 0.1-0.6."""
    return float(np.max(np.abs(cubic(c, GRID) - truth(GRID))))


def plant_tile_outliers(data, tiles, seed, frac=0.10):
    """A copy of float32 tile data with a fraction of every tile's pixels replaced by U(0, 1)."""
    rng = np.random.default_rng(seed)
    d = np.array(data, np.float32)
    for t in tiles:
        n = t.width * t.height * t.channels
        hit = rng.random(n) < frac
        v = d[t.offset:t.offset + n]
        v[hit] = rng.uniform(0, 1, int(hit.sum())).astype(np.float32)
    return d
