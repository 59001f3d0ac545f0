"""CPU restatement of the disparity-tile registration (csrc/pf_disp.hip): the fit of
y = 1/(a x + b) + d by the Ceres 1.13 trust-region LM in fp64, and D2DTransform in fp32.

TEST INFRASTRUCTURE ONLY.  The fit follows the kernel operation for operation: the sums are
taken in its documented order (lane l of 256 adds samples l, l + 256, ... in order from 0.0, then
the halving tree p[l] = p[l] + p[l + stride] for stride 128 ... 1) with elementwise numpy
operations and explicit ordered adds, and the scalar LM algebra runs on Python floats.  Every
operation is an IEEE-754 fp64 + - * / or sqrt, correctly rounded on both sides, so the two agree
bit for bit.
"""
import math

import numpy as np

LANES = 256
MAX_ITER = 50
INIT_RADIUS, MAX_RADIUS, MIN_RADIUS = 1e4, 1e16, 1e-32
MIN_REL_DECREASE, MIN_DIAG, MAX_DIAG = 1e-3, 1e-6, 1e32
MAX_INVALID = 5
FUNC_TOL, GRAD_TOL, PARAM_TOL = 1e-6, 1e-10, 1e-8
DBL_MAX = float(np.finfo(np.float64).max)
TERMINATION = ("no_convergence", "function_tolerance", "parameter_tolerance",
               "gradient_tolerance", "min_trust_region_radius", "failure")


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


def _inv_psd1(v):
    l = math.sqrt(v)
    return (1.0 / l) / l


def _llt2_solve(S, rhs):
    if not S[0][0] > 0.0:
        return None
    l00 = math.sqrt(S[0][0])
    l10 = S[0][1] / l00
    x = S[1][1] - l10 * l10
    if not x > 0.0:
        return None
    l11 = math.sqrt(x)
    y0 = rhs[0] / l00
    y1 = rhs[1] - l10 * y0
    y1 = y1 / l11
    y1 = y1 / l11
    y0 = y0 - l10 * y1
    y0 = y0 / l00
    return [y0, y1]


def _norm3(v):
    return math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])


def fit(xs, ys, trial_cost=None, trace=None):
    """The LM fit on already clamped samples.  Returns (coef64[4] = (a, b, 1, d), summary dict).

    trial_cost(p) (optional) replaces the trial evaluation; trace (optional list) receives one
    dict per iteration: the radius and parameters it started from and what became of the step.
    """
    xs = np.ascontiguousarray(xs, np.float64)
    ys = np.ascontiguousarray(ys, np.float64)
    if trial_cost is None:
        def trial_cost(p):
            return cost(xs, ys, p)
    x = [1.0, 1.0, 1.0]
    best = [1.0, 1.0, 1.0]
    S = sums(xs, ys, x)
    sc = [1.0 / (1.0 + math.sqrt(S[4])), 1.0 / (1.0 + math.sqrt(S[7])),
          1.0 / (1.0 + math.sqrt(S[9]))]

    def take(S):
        M = [[S[4], S[5], S[6]], [S[5], S[7], S[8]], [S[6], S[8], S[9]]]
        g = [S[1], S[2], S[3]]
        Ms = [[(M[i][j] * sc[i]) * sc[j] for j in range(3)] for i in range(3)]
        return g, Ms

    g, Ms = take(S)
    x_cost = S[0]
    initial_cost = x_cost
    radius, decrease, x_norm, min_cost = INIT_RADIUS, 2.0, -1.0, DBL_MAX
    reuse_diag, successful = False, True
    invalid_run, iteration, term = 0, 0, 0
    diag = [0.0, 0.0, 0.0]
    while True:
        if successful and x_cost < min_cost:
            min_cost = x_cost
            best = list(x)
        if iteration >= MAX_ITER:
            term = 0
            break
        if successful:
            gmax = 0.0
            for k in range(3):
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
        rec = {"iteration": iteration, "radius": radius, "x": tuple(x)}
        if trace is not None:
            trace.append(rec)
        if not reuse_diag:
            for k in range(3):
                d = Ms[k][k] if Ms[k][k] > MIN_DIAG else MIN_DIAG
                diag[k] = d if d < MAX_DIAG else MAX_DIAG
        D = [math.sqrt(diag[k] / radius) for k in range(3)]
        gs = [sc[k] * g[k] for k in range(3)]
        ete = D[0] * D[0] + Ms[0][0]
        R = [[0.0, 0.0], [0.0, 0.0]]
        for a in range(2):
            for c in range(a, 2):
                R[a][c] = Ms[1 + a][1 + c] + (D[1 + a] * D[1 + a] if a == c else 0.0)
        inv = _inv_psd1(ete)
        inv_g = inv * gs[0]
        rhs = [gs[1 + a] - Ms[0][1 + a] * inv_g for a in range(2)]
        for a in range(2):
            bt = Ms[0][1 + a] * inv
            for c in range(a, 2):
                R[a][c] = R[a][c] - bt * Ms[0][1 + c]
        z = _llt2_solve(R, rhs)
        ok = z is not None
        step = [0.0, 0.0, 0.0]
        if ok:
            ya = gs[0]
            for a in range(2):
                ya = ya - Ms[0][1 + a] * z[a]
            step = [inv * ya, z[0], z[1]]
            ok = all(math.isfinite(v) for v in step)
        reuse_diag = True
        mcc, cand_cost, valid = 0.0, 0.0, False
        if ok:
            step = [v * -1.0 for v in step]
            sJr, sMs = 0.0, 0.0
            for i in range(3):
                q = 0.0
                for j in range(3):
                    q = q + Ms[i][j] * step[j]
                sMs = sMs + step[i] * q
                sJr = sJr + step[i] * gs[i]
            mcc = -(sJr + sMs / 2.0)
            valid = mcc > 0.0
        if valid:
            cand = [x[k] + step[k] * sc[k] for k in range(3)]
            cand_cost = trial_cost(cand)
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
        dx = [x[k] - cand[k] for k in range(3)]
        if _norm3(dx) <= PARAM_TOL * (x_norm + PARAM_TOL):
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
            x_norm = _norm3(x)
            S = sums(xs, ys, x)
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
            rec["outcome"] = "rejected"
            radius = radius / decrease
            decrease *= 2.0
            successful = False
    coef = np.array([best[0], best[1], 1.0, best[2]], np.float64)
    summary = {"initial_cost": initial_cost, "final_cost": min_cost, "iterations": iteration,
               "termination": TERMINATION[term], "termination_code": term,
               "final_radius": radius, "x": tuple(x)}
    return coef, summary


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
