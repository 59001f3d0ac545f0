"""CPU restatement of the global result-to-baseline tools (csrc/pf_global.hip): the cubic fit of
SolveDepthToDepth2 (Depth.cpp:1158-1259) with the u16 result transform, MedianScaling
(Depth.cpp:637-701) and EquirectangularMap::CopyInvalidPixels (Depth.cpp:703-725).

TEST INFRASTRUCTURE ONLY.  The fit follows the kernels operation for operation: the 15 moment
sums are taken in their documented order (chunks of 16,384 consecutive samples; in a chunk lane l
of 256 adds its samples l, l + 256, ... in order from 0.0, then the halving tree
p[l] = p[l] + p[l + stride] for stride 128 ... 1; the chunk partials are added in chunk order
from 0.0) with elementwise numpy operations and explicit ordered adds, and the moment-form LM
(lm_moments of csrc/pf_register.hip, over lm_ref.solve) runs on Python floats from a start point.  Every operation is
an IEEE-754 fp64 + - * / or sqrt, correctly rounded on both sides, so the two agree bit for bit.
"""
import math

import numpy as np

import lm_ref

MYPI = 3.14159265359  # Basic.h:11
LANES = 256
CHUNK = 16384
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


def lm_moments(S, start=START_GLOBAL):
    """Ceres 1.13 trust-region LM (lm_ref.solve) on the 15 sums from `start`.
    Returns (coef64[4], summary dict)."""
    S = [float(v) for v in S]
    M = [[S[_IDX[i][j]] for j in range(4)] for i in range(4)]
    Jy = [S[10 + i] for i in range(4)]
    yy = S[14]
    best, summary = lm_ref.solve(
        start, lambda p: (_mom_cost(M, Jy, yy, p), _mom_gradient(M, Jy, p), M),
        lambda p: _mom_cost(M, Jy, yy, p), False)
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
