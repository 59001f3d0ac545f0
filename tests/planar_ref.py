"""CPU restatement of the planar-depth tile path (pf_set_tile_depth: csrc/pf_ray.hpp and the planar
instantiations of csrc/pf_register.hip, pf_robust.hip, pf_disp.hip).

TEST INFRASTRUCTURE ONLY.  A planar-depth tile holds depth along the optical axis; at tile pixel
(i, j) it differs from ray distance by kf(i, j) = float32(sqrt(1.0 + cu[i] + rv[j])), the adds and
the sqrt in fp64.  The registrations fit K T(x) to the baseline with K = float64(kf) of the pixel a
sample reads, and apply writes clamp01(kf * T32(x)) in fp32.  Everything here follows the kernels
operation for operation in IEEE-754 fp64 / fp32 + - * / sqrt, so the two agree bit for bit; the
only library function is tan in the tables, which the GPU tests allow 4 ulp.

  tables / kf            the layout's tables and factor in numpy
  sample_pixels / sample_K  the pixel every registration sample reads, from the oracle's own sample
                         walk (O.reg_samples on a tile that holds its pixel numbers), and its K
  reg_sums / register    the 15 (+1: the valid count) weighted moment sums in k_register's order,
                         solved by O.lm_moments or by the normal equations (solve_normal)
  fit                    the sample-wise cubic / disparity fit (lm_ref.solve) under the losses of
                         robust_ref, with the K-scaled residual and row
  apply_cubic / apply_disp  the fp32 transforms
"""
import math

import numpy as np

import disp_ref as DR
import lm_ref
import pyoracle as O
import robust_ref as RR
from lm_ref import TERMINATION

f32 = np.float32
LANES = 256
MODELS = RR.MODELS


# ---- tables and factor ------------------------------------------------------------------------
def tables(fov, w, h):
    """(cu float64 [w], rv float64 [h]) of a tile with viewing window fov = (az_left, az_right,
    zen_top, zen_down), as csrc/pf_ray.hpp builds them."""
    az_l, az_r, z_t, z_d = [f32(v) for v in fov]
    tx = math.tan(float(abs(f32(az_r - az_l))) / 2)
    ty = math.tan(float(abs(f32(z_t - z_d))) / 2)
    if w > 1:
        u = tx * (1 - 2 * np.arange(w, dtype=np.float64) / float(w - 1))
    else:
        u = np.zeros(w)
    if h > 1:
        v = ty * (2 * np.arange(h, dtype=np.float64) / float(h - 1) - 1)
    else:
        v = np.zeros(h)
    return u * u, v * v


def kf(cu, rv):
    """float32 [h][w]: the one definition of the factor."""
    return np.sqrt((1.0 + cu[None, :]) + rv[:, None]).astype(f32)


def layout_kf(layout):
    """[kf of tile p] from the layout's windows."""
    return [kf(*tables(layout.fovs[p], int(layout.tile_w[p]), int(layout.tile_h[p])))
            for p in range(layout.ntiles)]


def geometry_norm(tile):
    """float64 [h][w]: |corner0 + x hedge + y vedge| at x = i / (w-1), y = j / (h-1) from the
    oracle's fp32 tile geometry (SetWindow's plane at unit distance)."""
    c0, he, ve = [np.array(list(v), np.float64) for v in (tile.corner0, tile.hedge, tile.vedge)]
    x = np.arange(tile.width, dtype=np.float64) / (tile.width - 1)
    y = np.arange(tile.height, dtype=np.float64) / (tile.height - 1)
    pos = c0[None, None, :] + x[None, :, None] * he[None, None, :] + y[:, None, None] * ve
    return np.sqrt((pos * pos).sum(2))


# ---- the samples' pixels ------------------------------------------------------------------------
def sample_pixels(tile, emap, zr):
    """int64 [ns]: the pixel number Y * W + X every registration sample of the tile reads -- the
    oracle's own walk (O.reg_samples) over a tile holding 0.25 + 0.5 k / n at pixel k, which the
    sample clamp leaves alone and fp32 resolves for any n below 2^21."""
    n = tile.width * tile.height
    assert n < (1 << 21)
    ramp = np.zeros(tile.offset + n * tile.channels, f32)
    ramp[tile.offset::tile.channels][:n] = (0.25 + 0.5 * np.arange(n) / n).astype(f32)
    xs, _, _, _ = O.reg_samples(tile, ramp, np.ascontiguousarray(emap, f32), zr)
    k = (xs - 0.25) * (2.0 * n)
    pix = np.rint(k).astype(np.int64)
    assert np.abs(k - pix).max() < 0.25 and pix.min() >= 0 and pix.max() < n
    return pix


def sample_K(tile, emap, zr, kf_tile):
    """float64 [ns]: K = (double)kf of the pixel each sample reads."""
    return kf_tile.reshape(-1)[sample_pixels(tile, emap, zr)].astype(np.float64)


# ---- the moment form ----------------------------------------------------------------------------
def reg_terms(xs, ys, K):
    """The 16 terms of every sample, fp64 [ns][16]: k_register_planar's 15 with e = (K X^3, K X^2,
    K X, K) in place of (X^3, X^2, X, 1), then the count."""
    X = np.asarray(xs, np.float64)
    y = np.asarray(ys, np.float64)
    K = np.asarray(K, np.float64)
    X2 = X * X
    X3 = X * X * X
    e3, e2, e1, e0 = K * X3, K * X2, K * X, K
    return np.stack([e3 * e3, e3 * e2, e3 * e1, e3 * e0, e2 * e2, e2 * e1, e2 * e0, e1 * e1,
                     e1 * e0, e0 * e0, e3 * y, e2 * y, e1 * y, e0 * y, y * y,
                     np.ones_like(X)], 1)


def ordered_sums(T):
    """Column sums of fp64 [ns][m] in the kernels' order: lane l of 256 adds rows l, l + 256, ...
    from 0.0, then the halving tree 128 ... 1."""
    ns, m = T.shape
    rows = (ns + LANES - 1) // LANES
    P = np.zeros((rows * LANES, m), np.float64)
    P[:ns] = T
    P = P.reshape(rows, LANES, m)
    part = np.zeros((LANES, m), np.float64)
    for r in range(rows):
        part = part + P[r]
    stride = LANES // 2
    while stride >= 1:
        part[:stride] = part[:stride] + part[stride:2 * stride]
        stride //= 2
    return part[0].copy()


def reg_sums(xs, ys, K, valid=None):
    """The 16 sums of one tile; valid [ns] bool (None: all): a skipped sample adds 0.0 (every term
    is positive, so that changes no bit)."""
    if valid is not None:
        valid = np.asarray(valid, bool)
        xs = np.where(valid, xs, 0.5)
        ys = np.where(valid, ys, 0.5)
    T = reg_terms(xs, ys, K)
    if valid is not None:
        T = np.where(valid[:, None], T, 0.0)
    return ordered_sums(T)


_IDX = ((0, 1, 2, 3), (1, 4, 5, 6), (2, 5, 7, 8), (3, 6, 8, 9))


def solve_normal(S, degree):
    """solve_normal of csrc/pf_register.hip on Python floats: Gaussian elimination with partial
    pivoting on the degree + 1 lowest-order rows; None when a pivot is not positive."""
    n, off = degree + 1, 3 - degree
    A = [[float(S[_IDX[i + off][j + off]]) for j in range(n)] + [float(S[10 + i + off])]
         for i in range(n)]
    for k in range(n):
        piv, best = k, abs(A[k][k])
        for i in range(k + 1, n):
            if abs(A[i][k]) > best:
                best, piv = abs(A[i][k]), i
        if not best > 0.0:
            return None
        if piv != k:
            A[k], A[piv] = A[piv], A[k]
        for i in range(k + 1, n):
            f = A[i][k] / A[k][k]
            for j in range(k, n + 1):
                A[i][j] = A[i][j] - f * A[k][j]
    coef = [0.0] * n
    for i in range(n - 1, -1, -1):
        s = A[i][n]
        for j in range(i + 1, n):
            s = s - A[i][j] * coef[j]
        coef[i] = s / A[i][i]
    return coef


def solve_sums(S, degree=3, solver="lm", masked=False):
    """solve_store / solve_store_valid on the 16 sums: float64 [4] = (a, b, c, d)."""
    nan4 = np.full(4, np.nan)
    if masked and S[15] < degree + 1:
        return nan4
    if solver == "lm" and degree == 3:
        c, _ = O.lm_moments(S[:15])
    else:
        d, coef = degree, None
        while d >= 0 and coef is None:
            coef = solve_normal(S, d)
            if coef is None:
                d -= 1
        if coef is None:
            d, coef = 0, [0.0]
        c = np.zeros(4, np.float64)
        c[3 - d:] = coef
    if masked and not np.isfinite(c).all():
        return nan4
    return c


def register(xs, ys, K, valid=None, degree=3, solver="lm"):
    """The moment-form planar registration of one tile: (coef64 [4], sums [16])."""
    S = reg_sums(xs, ys, K, valid)
    return solve_sums(S, degree, solver, masked=valid is not None), S


# ---- the sample-wise form -----------------------------------------------------------------------
def residual_and_rows(xs, ys, K, p, model):
    """The residual K m - y and the Jacobian row's columns, each K times the plain one."""
    if model == "cubic":
        X2 = xs * xs
        X3 = xs * xs * xs
        r = K * (((X3 * p[0] + X2 * p[1]) + xs * p[2]) + p[3]) - ys
        return r, [K * X3, K * X2, K * xs, K]
    q = 1.0 / (p[0] * xs + p[1])
    qq = q * q
    r = K * (q + p[2]) - ys
    return r, [K * -(xs * qq), K * -qq, K]


def term_arrays(xs, ys, K, p, kind, a, model):
    """The per-sample terms of a Jacobian evaluation in the kernels' order: the cost term, the n of
    J'r, the n (n + 1) / 2 of upper J'J row by row.  kind None is the disparity fit without a loss
    (no weight is formed)."""
    with np.errstate(all="ignore"):
        r, J = residual_and_rows(xs, ys, K, p, model)
        if kind is None:
            rc, c0 = r, 0.5 * (r * r)
        else:
            rho0, rho1 = RR.loss(kind, a, r * r)
            w = np.sqrt(rho1)
            rc, c0 = w * r, 0.5 * rho0
            J = [w * j for j in J]
        n = len(J)
        terms = [c0] + [J[i] * rc for i in range(n)]
        terms += [J[i] * J[j] for i in range(n) for j in range(i, n)]
        return terms


def _masked(t, valid):
    return t if valid is None else np.where(valid, t, 0.0)


def sums(xs, ys, K, p, kind, a, model, valid=None):
    return [DR.ordered_sum(_masked(t, valid)) for t in term_arrays(xs, ys, K, p, kind, a, model)]


def cost(xs, ys, K, p, kind, a, model, valid=None):
    with np.errstate(all="ignore"):
        r, _ = residual_and_rows(xs, ys, K, p, model)
        c0 = 0.5 * (r * r) if kind is None else 0.5 * RR.loss(kind, a, r * r)[0]
        return DR.ordered_sum(_masked(c0, valid))


def fit(xs, ys, K, kind, a=0.0, model="cubic", valid=None):
    """The sample-wise LM fit on already clamped samples: robust_ref.fit with the ray factor.
    Returns (coef64 [4], summary dict); the disparity model's coefficients are (a, b, 1, d)."""
    xs = np.ascontiguousarray(xs, np.float64)
    ys = np.ascontiguousarray(ys, np.float64)
    K = np.ascontiguousarray(K, np.float64)
    n = MODELS[model]
    used = int(xs.size if valid is None else np.count_nonzero(valid))
    if valid is not None:
        valid = np.asarray(valid, bool)
        xs = np.where(valid, xs, 0.5)
        ys = np.where(valid, ys, 0.5)
    nan4 = np.full(4, np.nan)
    if valid is not None and used < 4:
        return nan4, {"initial_cost": math.nan, "final_cost": math.nan, "iterations": 0,
                      "termination_code": 5, "termination": TERMINATION[5], "used": used,
                      "inliers": 0}
    best, summary = lm_ref.solve(
        [1.0] * n,
        lambda p: lm_ref.unpack_sums(sums(xs, ys, K, p, kind, a, model, valid), n),
        lambda p: cost(xs, ys, K, p, kind, a, model, valid), True)
    with np.errstate(all="ignore"):
        r, _ = residual_and_rows(xs, ys, K, best, model)
        inl = (r * r) <= a * a
        if valid is not None:
            inl = inl & valid
    if model == "cubic":
        coef = np.array(best, np.float64)
        if not all(math.isfinite(v) for v in best):
            coef = nan4
            summary.update(termination_code=5, termination=TERMINATION[5])
    else:
        coef = np.array([best[0], best[1], 1.0, best[2]], np.float64)
    summary.update(used=used, inliers=int(np.count_nonzero(inl)))
    return coef, summary


# ---- apply --------------------------------------------------------------------------------------
def _clamp_x(data):
    X = np.asarray(data, f32).copy()
    wide = X.astype(np.float64)
    lo = wide < 1e-4
    hi = ~lo & (wide > (1 - 1e-4))
    X[lo] = f32(1e-4)
    X[hi] = f32(1 - 1e-4)
    return X


def _finish(Y, kf_tile, raw, valid):
    Y = (kf_tile.reshape(-1) * Y).astype(f32)
    neg = Y < 0
    big = ~neg & (Y > 1)
    Y[neg] = f32(0)
    Y[big] = f32(1)
    if valid is not None:
        lo, hi = f32(valid[0]), f32(valid[1])
        with np.errstate(invalid="ignore"):
            ok = (lo < raw) & (raw < hi)
        Y[~ok] = f32(np.nan)
    return Y


def apply_cubic(data, abcd, kf_tile, valid=None):
    """clamp01(kf * T32(x)) of one tile's float32 pixels (flat), T32 = Depth2DepthTransform before
    its final clamp; valid = (lo, hi): a pixel failing the rule becomes NaN.  A new array."""
    raw = np.asarray(data, f32).reshape(-1)
    a, b, c, d = [f32(v) for v in np.asarray(abcd, f32)]
    X = _clamp_x(raw)
    with np.errstate(all="ignore"):
        Y = (a * X * X * X + b * X * X + c * X + d).astype(f32)
        return _finish(Y, kf_tile, raw, valid)


def apply_disp(data, abcd, kf_tile):
    """The same with D2DTransform: T32 = c / (a X + b) + d."""
    raw = np.asarray(data, f32).reshape(-1)
    a, b, c, d = [f32(v) for v in np.asarray(abcd, f32)]
    X = _clamp_x(raw)
    with np.errstate(all="ignore"):
        Y = (c / (a * X + b) + d).astype(f32)
        return _finish(Y, kf_tile, raw, None)


def apply_all(tiles, data, abcd, kfs, model="cubic", valid=None):
    """Every tile of a layout (channel 0 of one-channel tiles): a new flat float32 array."""
    out = np.array(data, f32)
    for p, t in enumerate(tiles):
        n = t.width * t.height
        seg = out[t.offset:t.offset + n]
        if model == "cubic":
            out[t.offset:t.offset + n] = apply_cubic(seg, abcd[p], kfs[p], valid)
        else:
            out[t.offset:t.offset + n] = apply_disp(seg, abcd[p], kfs[p])
    return out
