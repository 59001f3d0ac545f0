"""CPU restatement of the global result-to-baseline tools (csrc/pf_global.hip): the cubic fit of
SolveDepthToDepth2 (Depth.cpp:1158-1259) with the u16 result transform, MedianScaling
(Depth.cpp:637-701) and EquirectangularMap::CopyInvalidPixels (Depth.cpp:703-725).

TEST INFRASTRUCTURE ONLY.  The fit follows the kernels operation for operation: the 15 moment
sums are taken in their documented order (chunks of 16,384 consecutive samples; in a chunk lane l
of 256 adds its samples l, l + 256, ... in order from 0.0, then the halving tree
p[l] = p[l] + p[l + stride] for stride 128 ... 1; the chunk partials are added in chunk order
from 0.0) with elementwise numpy operations and explicit ordered adds, and the moment-form LM
(lm_moments of csrc/pf_kernels.hip) runs on Python floats from a start point.  Every operation is
an IEEE-754 fp64 + - * / or sqrt, correctly rounded on both sides, so the two agree bit for bit.
"""
import math

import numpy as np

MYPI = 3.14159265359  # Basic.h:11
LANES = 256
CHUNK = 16384
MAX_ITER = 50
INIT_RADIUS, MAX_RADIUS, MIN_RADIUS = 1e4, 1e16, 1e-32
MIN_REL_DECREASE, MIN_DIAG, MAX_DIAG = 1e-3, 1e-6, 1e32
MAX_INVALID = 5
FUNC_TOL, GRAD_TOL, PARAM_TOL = 1e-6, 1e-10, 1e-8
DBL_MAX = float(np.finfo(np.float64).max)
TERMINATION = ("no_convergence", "function_tolerance", "parameter_tolerance",
               "gradient_tolerance", "min_trust_region_radius", "failure")
START_GLOBAL = (0.0, 0.0, 1.0, 0.0)  # Depth.cpp:1169-1173
START_TILE = (1.0, 1.0, 1.0, 1.0)    # Depth.cpp:1270-1274

f32 = np.float32


# ---------------------------------------------------------------------------------------------
# samples
def band(height, zr):
    """(h0, h1) of SolveDepthToDepth2 (Depth.cpp:1166-1167): int * float in fp32, / MYPI in fp64."""
    h0 = math.floor(float(f32(height) * f32(zr[0])) / MYPI)
    h1 = math.ceil(float(f32(height) * f32(zr[1])) / MYPI)
    return int(h0), int(h1)


def emap_tables(width, height, ew, eh):
    """ValueAtCoord's column index per X and row index per Y (Depth.cpp:1198, 551-556)."""
    X = np.arange(width, dtype=np.float32)
    Y = np.arange(height + 1, dtype=np.float32)  # the band may end at row `height`
    az = ((X / f32(width - 1) * f32(2)).astype(np.float64) * MYPI).astype(np.float32)
    zen = ((Y / f32(height - 1)).astype(np.float64) * MYPI).astype(np.float32)
    col = (az.astype(np.float64) / (MYPI * 2) * float(f32(ew - 1))).astype(np.int64)
    row = (zen.astype(np.float64) / MYPI * float(f32(eh - 1))).astype(np.int64)
    return col, row


def clamp_samples(v):
    """The clamp to [1e-4, 1 - 1e-4] with the source's double literals (Depth.cpp:1200-1210)."""
    v = np.asarray(v, np.float64).copy()
    lo = v < 1e-4
    hi = ~lo & (v > (1 - 1e-4))
    v[lo] = 1e-4
    v[hi] = 1 - 1e-4
    return v


def samples(emap, data, zr):
    """(xs, ys) fp64, clamped, in sample order s = (Y - h0) * W + X.
    emap: float32 [eh][ew] or [eh][ew][ec]; data: uint16 [H][W]."""
    emap = np.asarray(emap, np.float32)
    if emap.ndim == 2:
        emap = emap[:, :, None]
    data = np.asarray(data, np.uint16)
    H, W = data.shape
    eh, ew = emap.shape[:2]
    h0, h1 = band(H, zr)
    if not (0 <= h0 <= h1 <= H - 1):
        raise ValueError(f"band {h0}..{h1} outside the {H} rows")
    col, row = emap_tables(W, H, ew, eh)
    x = (data[h0:h1 + 1].astype(np.float32) / f32(65535.0)).astype(np.float64)
    y = emap[row[h0:h1 + 1]][:, col, 0].astype(np.float64)
    return clamp_samples(x.ravel()), clamp_samples(y.ravel())


# ---------------------------------------------------------------------------------------------
# sums
def _chunk_sum(terms):
    n = terms.size
    rows = (n + LANES - 1) // LANES
    acc = np.zeros(LANES, np.float64)
    for r in range(rows):
        part = terms[r * LANES:(r + 1) * LANES]
        acc[:part.size] = acc[:part.size] + part
    stride = LANES // 2
    while stride >= 1:
        acc[:stride] = acc[:stride] + acc[stride:2 * stride]
        stride //= 2
    return float(acc[0])


def ordered_sum(terms):
    """Sum of a 1-D fp64 array in the kernels' order."""
    total = 0.0
    for c0 in range(0, terms.size, CHUNK):
        total = total + _chunk_sum(terms[c0:c0 + CHUNK])
    return total


def moment_terms(xs, ys):
    """The 15 per-sample products of k_register (kRegSums), same products, same order."""
    X, Y = xs, ys
    X2 = X * X
    X3 = X * X * X
    return (X3 * X3, X3 * X2, X3 * X, X3, X2 * X2, X2 * X, X2, X * X, X, np.ones_like(X),
            X3 * Y, X2 * Y, X * Y, Y, Y * Y)


def moment_sums(xs, ys):
    return [ordered_sum(t) for t in moment_terms(xs, ys)]


# ---------------------------------------------------------------------------------------------
# the moment-form LM (lm_moments)
_IDX = ((0, 1, 2, 3), (1, 4, 5, 6), (2, 5, 7, 8), (3, 6, 8, 9))


def _mom_cost(M, Jy, yy, p):
    pMp, pJy = 0.0, 0.0
    for i in range(4):
        q = 0.0
        for j in range(4):
            q = q + M[i][j] * p[j]
        pMp = pMp + p[i] * q
        pJy = pJy + p[i] * Jy[i]
    return 0.5 * ((yy - 2.0 * pJy) + pMp)


def _mom_gradient(M, Jy, p):
    g = [0.0] * 4
    for i in range(4):
        q = 0.0
        for j in range(4):
            q = q + M[i][j] * p[j]
        g[i] = q - Jy[i]
    return g


def _inv_psd1(v):
    l = math.sqrt(v)
    return (1.0 / l) / l


def _llt3_solve(S, rhs):
    L = [[0.0] * 3 for _ in range(3)]
    for k in range(3):
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
        for j in range(k + 1, 3):
            a = S[k][j]
            for i in range(k):
                a = a - L[j][i] * L[k][i]
            L[j][k] = a / x
    y = list(rhs)
    for k in range(3):
        y[k] = y[k] / L[k][k]
        for j in range(k + 1, 3):
            y[j] = y[j] - L[j][k] * y[k]
    for k in (2, 1, 0):
        y[k] = y[k] / L[k][k]
        for j in range(k):
            y[j] = y[j] - L[k][j] * y[k]
    return y


def _norm4(v):
    return math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3])


def _sqrt(v):
    return math.sqrt(v) if v >= 0.0 else float("nan")


def lm_moments(S, start=START_GLOBAL):
    """Ceres 1.13 trust-region LM (DENSE_SCHUR, default options) on the 15 sums from `start`.
    Returns (coef64[4], summary dict)."""
    S = [float(v) for v in S]
    M = [[S[_IDX[i][j]] for j in range(4)] for i in range(4)]
    Jy = [S[10 + i] for i in range(4)]
    yy = S[14]
    x = [float(v) for v in start]
    best = list(x)
    sc = [1.0 / (1.0 + _sqrt(M[k][k])) for k in range(4)]
    Ms = [[(M[i][j] * sc[i]) * sc[j] for j in range(4)] for i in range(4)]
    radius, decrease, x_norm = INIT_RADIUS, 2.0, -1.0
    reuse_diag, successful = False, True
    invalid_run, iteration, term = 0, 0, 0
    diag = [0.0] * 4
    x_cost = _mom_cost(M, Jy, yy, x)
    g = _mom_gradient(M, Jy, x)
    initial_cost = x_cost
    min_cost = DBL_MAX
    while True:
        if successful and x_cost < min_cost:
            min_cost = x_cost
            best = list(x)
        if iteration >= MAX_ITER:
            term = 0
            break
        if successful:
            gmax = 0.0
            for k in range(4):
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
        if not reuse_diag:
            for k in range(4):
                d = Ms[k][k] if Ms[k][k] > MIN_DIAG else MIN_DIAG
                diag[k] = d if d < MAX_DIAG else MAX_DIAG
        D = [math.sqrt(diag[k] / radius) for k in range(4)]
        gs = [sc[k] * g[k] for k in range(4)]
        ete = D[0] * D[0] + Ms[0][0]
        R = [[0.0] * 3 for _ in range(3)]
        for a in range(3):
            for b in range(a, 3):
                R[a][b] = Ms[1 + a][1 + b] + (D[1 + a] * D[1 + a] if a == b else 0.0)
        inv = _inv_psd1(ete)
        inv_g = inv * gs[0]
        rhs = [gs[1 + a] - Ms[0][1 + a] * inv_g for a in range(3)]
        for a in range(3):
            bt = Ms[0][1 + a] * inv
            for b in range(a, 3):
                R[a][b] = R[a][b] - bt * Ms[0][1 + b]
        z = _llt3_solve(R, rhs)
        ok = z is not None
        step = [0.0] * 4
        if ok:
            ya = gs[0]
            for a in range(3):
                ya = ya - Ms[0][1 + a] * z[a]
            step = [inv * ya, z[0], z[1], z[2]]
            ok = all(math.isfinite(v) for v in step)
        reuse_diag = True
        mcc, valid = 0.0, False
        if ok:
            step = [v * -1.0 for v in step]
            sJr, sMs = 0.0, 0.0
            for i in range(4):
                q = 0.0
                for j in range(4):
                    q = q + Ms[i][j] * step[j]
                sMs = sMs + step[i] * q
                sJr = sJr + step[i] * gs[i]
            mcc = -(sJr + sMs / 2.0)
            valid = mcc > 0.0
        if not valid:
            invalid_run += 1
            if invalid_run >= MAX_INVALID:
                term = 5
                break
            radius = radius / decrease
            decrease *= 2.0
            successful = False
            continue
        invalid_run = 0
        cand = [x[k] + step[k] * sc[k] for k in range(4)]
        cand_cost = _mom_cost(M, Jy, yy, cand)
        if not math.isfinite(cand_cost):
            cand_cost = DBL_MAX
        dx = [x[k] - cand[k] for k in range(4)]
        if _norm4(dx) <= PARAM_TOL * (x_norm + PARAM_TOL):
            term = 2
            break
        if abs(x_cost - cand_cost) <= FUNC_TOL * x_cost:
            term = 1
            break
        rel = (x_cost - cand_cost) / mcc
        if rel > MIN_REL_DECREASE:
            x = list(cand)
            x_norm = _norm4(x)
            x_cost = _mom_cost(M, Jy, yy, x)
            g = _mom_gradient(M, Jy, x)
            q = 2.0 * rel - 1.0
            f = 1.0 - q * q * q
            radius = radius / (f if f > 1.0 / 3.0 else 1.0 / 3.0)
            radius = radius if radius < MAX_RADIUS else MAX_RADIUS
            decrease = 2.0
            reuse_diag = False
            successful = True
        else:
            radius = radius / decrease
            decrease *= 2.0
            successful = False
    summary = {"initial_cost": initial_cost, "final_cost": min_cost, "iterations": iteration,
               "termination": TERMINATION[term], "termination_code": term}
    return np.array(best, np.float64), summary


def summary_row(summary):
    """The kernel's summary: 4 doubles."""
    return np.array([summary["initial_cost"], summary["final_cost"],
                     float(summary["iterations"]), float(summary["termination_code"])],
                    np.float64)


def register_global(emap, data, zr):
    """SolveDepthToDepth2: (coef64[4], abcd float32[4] = Vec4f(vars), summary)."""
    xs, ys = samples(emap, data, zr)
    c64, s = lm_moments(moment_sums(xs, ys), START_GLOBAL)
    return c64, c64.astype(np.float32), s


# ---------------------------------------------------------------------------------------------
# the u16 result transform
def cubic_map(X, abcd):
    """Depth2DepthTransform's per-value map (Depth.cpp:256-271) of a float32 array in fp32."""
    a, b, c, d = [f32(v) for v in np.asarray(abcd, np.float32)]
    X = np.asarray(X, np.float32).copy()
    wide = X.astype(np.float64)
    lo = wide < 1e-4
    hi = ~lo & (wide > (1 - 1e-4))
    X[lo] = f32(1e-4)
    X[hi] = f32(1 - 1e-4)
    with np.errstate(all="ignore"):
        Y = (a * X * X * X + b * X * X + c * X + d).astype(np.float32)
    neg = Y < 0
    big = ~neg & (Y > 1)
    Y[neg] = f32(0)
    Y[big] = f32(1)
    return Y


def result_transform(data, zr, abcd):
    """Rows h0..h1 of a uint16 [H][W] result through the cubic: a new array.  NaN becomes 0."""
    data = np.asarray(data, np.uint16)
    out = data.copy()
    h0, h1 = band(data.shape[0], zr)
    v = data[h0:h1 + 1].astype(np.float32) / f32(65535.0)
    Y = cubic_map(v, abcd)
    Y = np.where(np.isnan(Y), f32(0), Y)
    out[h0:h1 + 1] = (Y * f32(65535.0)).astype(np.float32).astype(np.uint16)
    return out


# ---------------------------------------------------------------------------------------------
# MedianScaling, CopyInvalidPixels
def _chan0(m):
    m = np.asarray(m, np.float32)
    return m if m.ndim == 2 else m[:, :, 0]


def valid_mask(v):
    """!(v < 1e-4 || v >= 1 - 1e-4) with v promoted to double; NaN is invalid."""
    w = np.asarray(v, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return ~((w < 1e-4) | (w >= 1 - 1e-4)) & ~np.isnan(w)


def median_of(m):
    """The order statistic at index n/2 of channel 0's valid values, or None without any."""
    v = _chan0(m)
    vals = np.sort(v[valid_mask(v)])
    return None if vals.size == 0 else f32(vals[vals.size // 2])


def median_scale(map0, map1):
    """(ok, m0, m1, scaled map0): map0 * (m1 / m0) in fp32 on its valid pixels of channel 0.
    Without a valid pixel in either map: (False, 0, 0, map0 unchanged)."""
    out = np.asarray(map0, np.float32).copy()
    m0, m1 = median_of(map0), median_of(map1)
    if m0 is None or m1 is None:
        return False, f32(0), f32(0), out
    scaling = f32(m1) / f32(m0)
    c0 = out if out.ndim == 2 else out[:, :, 0]
    ok = valid_mask(c0)
    c0[ok] = (c0[ok] * scaling).astype(np.float32)
    return True, m0, m1, out


def copy_invalid(dst, ref):
    """CopyInvalidPixels: a new array."""
    out = np.asarray(dst, np.float32).copy()
    r = _chan0(ref)
    h, w = out.shape[:2]
    rh, rw = r.shape
    rx, ry = f32(rw) / f32(w), f32(rh) / f32(h)
    X = (np.arange(w, dtype=np.float32) * rx).astype(np.float32).astype(np.int64)
    Y = (np.arange(h, dtype=np.float32) * ry).astype(np.float32).astype(np.int64)
    val = r[np.ix_(Y, X)]
    wide = val.astype(np.float64)
    with np.errstate(invalid="ignore"):
        bad = (wide < 1e-4) | (wide >= 1 - 1e-4)
    c0 = out if out.ndim == 2 else out[:, :, 0]
    c0[bad] = val[bad]
    return out


def ulp_diff(a, b):
    """Per-element distance of two float32 arrays in units in the last place."""
    def key(v):
        u = np.asarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(u < 0, -(u & 0x7FFFFFFF), u)
    return np.abs(key(a) - key(b))
