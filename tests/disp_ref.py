"""CPU restatement of the disparity-tile registration (csrc/pf_disp.hip): the fit of
y = 1/(a x + b) + d by the Ceres 1.13 trust-region LM in fp64, and D2DTransform in fp32.

TEST INFRASTRUCTURE ONLY.  The fit follows the kernel operation for operation: the sums are
taken in its documented order (lane l of 256 adds samples l, l + 256, ... in order from 0.0, then
the halving tree p[l] = p[l] + p[l + stride] for stride 128 ... 1) with elementwise numpy
operations and explicit ordered adds, and the scalar LM algebra (lm_ref.solve) runs on Python floats.  Every
operation is an IEEE-754 fp64 + - * / or sqrt, correctly rounded on both sides, so the two agree
bit for bit.
"""
import numpy as np

import lm_ref
from lm_ref import DBL_MAX, MAX_INVALID, MAX_ITER, TERMINATION  # noqa: F401  (read by the tests)

LANES = 256


def clamp_samples(v):
    """SolveDepthToDepth's clamp of a sample value to [1e-4, 1 - 1e-4] (Depth.cpp:1352-1362)."""
    v = np.asarray(v, np.float64).copy()
    lo = v < 1e-4
    hi = ~lo & (v > (1 - 1e-4))
    v[lo] = 1e-4
    v[hi] = 1 - 1e-4
    return v


def ordered_sum(terms):
    """Sum of a 1-D fp64 array in the kernel's order."""
    n = terms.size
    rows = (n + LANES - 1) // LANES
    acc = np.zeros(LANES, np.float64)
    for r in range(rows):
        chunk = terms[r * LANES:(r + 1) * LANES]
        acc[:chunk.size] = acc[:chunk.size] + chunk
    stride = LANES // 2
    while stride >= 1:
        acc[:stride] = acc[:stride] + acc[stride:2 * stride]
        stride //= 2
    return float(acc[0])


def _residual(xs, ys, p):
    q = 1.0 / (p[0] * xs + p[1])
    return q, (q + p[2]) - ys


def cost(xs, ys, p):
    """0.5 sum r^2 at p = (a, b, d): a trial evaluation (one sum)."""
    with np.errstate(all="ignore"):
        _, r = _residual(xs, ys, p)
        return ordered_sum(0.5 * (r * r))


def sums(xs, ys, p):
    """The 10 sums of a Jacobian evaluation: cost, J'r (3), upper J'J (6)."""
    with np.errstate(all="ignore"):
        q, r = _residual(xs, ys, p)
        qq = q * q
        j0 = -(xs * qq)
        j1 = -qq
        one = np.ones_like(xs)
        terms = (0.5 * (r * r), j0 * r, j1 * r, r, j0 * j0, j0 * j1, j0, j1 * j1, j1, one)
        return [ordered_sum(t) for t in terms]


def fit(xs, ys, trial_cost=None, trace=None):
    """The LM fit (lm_ref.solve) on already clamped samples.  Returns (coef64[4] = (a, b, 1, d),
    summary dict).

    trial_cost(p) (optional) replaces the trial evaluation; trace (optional list) receives
    lm_ref.solve's record of every iteration.
    """
    xs = np.ascontiguousarray(xs, np.float64)
    ys = np.ascontiguousarray(ys, np.float64)
    if trial_cost is None:
        def trial_cost(p):
            return cost(xs, ys, p)
    best, summary = lm_ref.solve([1.0, 1.0, 1.0],
                                 lambda p: lm_ref.unpack_sums(sums(xs, ys, p), 3), trial_cost,
                                 True, trace)
    return np.array([best[0], best[1], 1.0, best[2]], np.float64), summary


def summary_row(summary):
    """The kernel's per-tile summary: 4 doubles."""
    return np.array([summary["initial_cost"], summary["final_cost"],
                     float(summary["iterations"]), float(summary["termination_code"])],
                    np.float64)


def register_tile(tile, tile_data, emap, zr):
    """The fit on SolveDepthToDepth's samples of one tile (pyoracle.reg_samples, already clamped):
    (coef64[4], abcd float32[4], summary)."""
    import pyoracle as O
    xs, ys, _, _ = O.reg_samples(tile, tile_data, emap, zr)
    c64, s = fit(xs, ys)
    return c64, c64.astype(np.float32), s


def transform(data, abcd):
    """D2DTransform (Depth.cpp:214-243) of a float32 array in fp32: a new array."""
    a, b, c, d = [np.float32(v) for v in np.asarray(abcd, np.float32)]
    X = np.asarray(data, np.float32).copy()
    wide = X.astype(np.float64)
    lo = wide < 1e-4
    hi = ~lo & (wide > (1 - 1e-4))
    X[lo] = np.float32(1e-4)
    X[hi] = np.float32(1 - 1e-4)
    with np.errstate(all="ignore"):
        Y = c / (a * X + b) + d
    Y = Y.astype(np.float32)
    neg = Y < 0
    big = ~neg & (Y > 1)
    Y[neg] = np.float32(0)
    Y[big] = np.float32(1)
    return Y
