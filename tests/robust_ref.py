"""CPU restatement of the robust tile registration (csrc/pf_robust.hip, and the loss instantiation
of csrc/pf_disp.hip): the sample-wise Ceres 1.13 trust-region LM of the cubic
y = a x^3 + b x^2 + c x + d, or of y = 1/(a x + b) + d, under HuberLoss or SoftLOneLoss.

TEST INFRASTRUCTURE ONLY.  The fit follows the kernels operation for operation: every sum is taken
by disp_ref.ordered_sum (lane l of 256 adds samples l, l + 256, ... in order from 0.0, then the
halving tree) over elementwise numpy fp64 terms, and the scalar LM algebra (lm_ref.solve) runs on
Python floats.
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
import lm_ref
from lm_ref import TERMINATION

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


def fit(xs, ys, kind, a=0.0, model="cubic", valid=None, trace=None, ordered_sum=None):
    """The LM fit on already clamped samples under the loss (kind None: plain least squares in the
    same sample-wise form).  valid: bool [ns] or None, the samples the validity rule keeps.
    Returns (coef64[4], summary dict); the disparity model's coefficients are (a, b, 1, d).
    trace (optional list) receives lm_ref.solve's record of every iteration."""
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
    best, summary = lm_ref.solve(
        [1.0] * n,
        lambda p: lm_ref.unpack_sums(sums(xs, ys, p, kind, a, model, valid, ordered_sum), n),
        lambda p: cost(xs, ys, p, kind, a, model, valid, ordered_sum), True, trace)
    with np.errstate(all="ignore"):
        r, _ = residual_and_rows(xs, ys, best, model)
        inl = (r * r) <= a * a
        if valid is not None:
            inl = inl & valid
    if model == "cubic":
        coef = np.array(best, np.float64)
        if not all(math.isfinite(v) for v in best):  # k_register_robust's guard
            coef = nan4
            summary.update(termination_code=5, termination=TERMINATION[5])
    else:
        coef = np.array([best[0], best[1], 1.0, best[2]], np.float64)
    summary.update(used=used, inliers=int(np.count_nonzero(inl)))
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
