"""CPU restatement of the weighted disparity-tile path (pf_tile_range_weights,
pf_register_disparity_weighted, pf_merge_disparity_weighted), built from tests/disp_ref.py (the
fit's terms, summation order and transform), tests/planar_ref.py (the planar terms, K and apply)
and tests/weight_ref.py (the usable weight, the samples' elements and the weighted fusion), none of
which is edited.

TEST INFRASTRUCTURE ONLY.  tests/test_disp_weight_ref.py proves the restatement; tests/
test_gpu_disp_weights.py holds the library to it bit for bit.

Usable weight.  u(w) = w if 0 < w < +inf in fp32, else 0 (weight_ref.usable).

Used sample.  Sample s of a tile is used iff u(w) > 0 at the tile element it reads, the raw tile
value there is finite and its baseline value is finite (the baseline is tested after the sample
clamp, which keeps a NaN; no test here feeds an infinite baseline).  W = float64(u(w)).

Sums.  Lane l of 256 owns samples l, l + 256, ... used or not; a used sample adds W * t_k, one
fp64 multiply and one fp64 add, t_k the ten terms of disp_ref.sums (planar_ref.term_arrays under
planar depth) in their order; a trial adds W * (0.5 * (r * r)).  A sample that is not used adds
nothing: here it adds +0.0 to a lane sum that starts at +0.0 and can never be -0.0 (x + (-x) is
+0.0 in round-to-nearest), which changes no bit.  Then disp_ref.ordered_sum's halving tree.  The
count of used samples and the sum of W go through the same lanes and tree.

Fit.  lm_ref.solve from (1, 1, 1) with non-finite trials invalid, as disp_ref.fit.  Fewer than 3
used samples: no fit, coefficients NaN, costs NaN, 0 iterations, termination 5.  A solution that
is not finite: coefficients NaN, termination 5, the other summary entries as the LM left them.

Merge.  The tiles transformed by the float32 coefficients (disp_ref.transform, or
planar_ref.apply_disp), every pixel; then weight_ref.fuse(..., transformed copy, weights,
abcd=None).  A tile with NaN coefficients is all NaN and weight_ref.staged drops it.
"""
import math

import numpy as np

import disp_ref as DR
import lm_ref
import planar_ref as P
import pyoracle as O
import weight_ref as WR
from lm_ref import TERMINATION

f32 = np.float32
ZR = WR.ZR
MIN_USED = 3


def range_weights(data, lo, hi, channels=1):
    """pf_tile_range_weights of float32 [..., tile_elems]: 1.0 at the channel-0 element of a pixel
    with lo < v < hi in fp32 (NaN fails), 0.0 everywhere else."""
    d = np.asarray(data, f32)
    out = np.zeros(d.shape, f32)
    with np.errstate(invalid="ignore"):
        ok = (f32(lo) < d) & (d < f32(hi))
    out[..., ::channels] = ok[..., ::channels].astype(f32)
    return out


def tile_samples(tile, data, weights, emap, zr=ZR):
    """(xs, ys clamped float64, W float64, used bool, elements) of one tile's samples."""
    data = np.ascontiguousarray(data, f32)
    el = WR.sample_elements(tile, emap, zr)
    raw = data[tile.offset + el]
    xs, ys, _, _ = O.reg_samples(tile, data, np.ascontiguousarray(emap, f32), zr)
    w = WR.usable(np.asarray(weights, f32).ravel()[tile.offset + el])
    used = (w > 0) & np.isfinite(raw) & np.isfinite(ys)
    return xs, ys, w.astype(np.float64), used, el


def _terms(xs, ys, K, p):
    """The ten per-sample terms of a Jacobian evaluation (disp_ref.sums' / planar_ref's)."""
    if K is not None:
        return P.term_arrays(xs, ys, K, p, None, 0.0, "disparity")
    with np.errstate(all="ignore"):
        q, r = DR._residual(xs, ys, p)
        qq = q * q
        j0 = -(xs * qq)
        j1 = -qq
        return [0.5 * (r * r), j0 * r, j1 * r, r, j0 * j0, j0 * j1, j0, j1 * j1, j1,
                np.ones_like(xs)]


def _weighted(t, W, used):
    with np.errstate(all="ignore"):
        return np.where(used, W * t, 0.0)


def sums(xs, ys, W, used, p, K=None):
    """The 10 weighted sums of a Jacobian evaluation at p = (a, b, d)."""
    return [DR.ordered_sum(_weighted(t, W, used)) for t in _terms(xs, ys, K, p)]


def cost(xs, ys, W, used, p, K=None):
    """The weighted trial cost: one sum."""
    with np.errstate(all="ignore"):
        q = 1.0 / (p[0] * xs + p[1])
        r = (q + p[2]) - ys if K is None else K * (q + p[2]) - ys
        return DR.ordered_sum(_weighted(0.5 * (r * r), W, used))


def fit(xs, ys, W, used, K=None):
    """The weighted fit on already clamped samples: (coef64 [4] = (a, b, 1, d), summary dict with
    `used` and `sum_w` added)."""
    xs = np.ascontiguousarray(xs, np.float64)
    ys = np.ascontiguousarray(ys, np.float64)
    W = np.ascontiguousarray(W, np.float64)
    used = np.asarray(used, bool)
    if K is not None:
        K = np.ascontiguousarray(K, np.float64)
    n_used = DR.ordered_sum(used.astype(np.float64))
    sum_w = DR.ordered_sum(np.where(used, W, 0.0))
    nan4 = np.full(4, np.nan)
    if n_used < MIN_USED:
        return nan4, {"initial_cost": math.nan, "final_cost": math.nan, "iterations": 0,
                      "termination_code": 5, "termination": TERMINATION[5], "used": n_used,
                      "sum_w": sum_w}
    # a sample that is not used never enters the arithmetic: park it inside the clamp range
    xs = np.where(used, xs, 0.5)
    ys = np.where(used, ys, 0.5)
    best, summary = lm_ref.solve(
        [1.0, 1.0, 1.0], lambda p: lm_ref.unpack_sums(sums(xs, ys, W, used, p, K), 3),
        lambda p: cost(xs, ys, W, used, p, K), True)
    coef = np.array([best[0], best[1], 1.0, best[2]], np.float64)
    if not all(math.isfinite(v) for v in best):
        coef = nan4
        summary.update(termination_code=5, termination=TERMINATION[5])
    summary.update(used=n_used, sum_w=sum_w)
    return coef, summary


def summary_row(s):
    """The kernel's per-tile summary: 6 doubles."""
    return np.array([s["initial_cost"], s["final_cost"], float(s["iterations"]),
                     float(s["termination_code"]), float(s["used"]), float(s["sum_w"])],
                    np.float64)


def register(tiles, data, weights, emap, zr=ZR, kfs=None):
    """(coeffs64 [n][4], summary [n][6]) of every tile of one panorama; kfs: the tiles' ray factor
    (planar_ref.layout_kf) under planar depth."""
    n = len(tiles)
    c64 = np.full((n, 4), np.nan, np.float64)
    summ = np.zeros((n, 6), np.float64)
    for p, t in enumerate(tiles):
        xs, ys, W, used, el = tile_samples(t, data, weights, emap, zr)
        K = None
        if kfs is not None:
            K = kfs[p].reshape(-1)[el // t.channels].astype(np.float64)
        c64[p], s = fit(xs, ys, W, used, K)
        summ[p] = summary_row(s)
    return c64, summ


def transform_all(tiles, data, abcd, kfs=None):
    """apply: D2DTransform (composed with the ray factor under planar depth) of channel 0 of every
    pixel of every tile: a new flat float32 array."""
    out = np.array(data, f32).ravel()
    for p, t in enumerate(tiles):
        sl = slice(t.offset, t.offset + t.width * t.height * t.channels, t.channels)
        if kfs is None:
            out[sl] = DR.transform(out[sl], abcd[p])
        else:
            out[sl] = P.apply_disp(out[sl], abcd[p], kfs[p])
    return out


def merge(emap, tiles, data, weights, out_w=WR.M.OUT_W, zr=ZR, kfs=None):
    """(u16 [out_w / 2][out_w], abcd float32 [n][4]) of pf_merge_disparity_weighted."""
    c64, _ = register(tiles, data, weights, emap, zr, kfs)
    abcd = c64.astype(f32)
    copy = transform_all(tiles, data, abcd, kfs)
    return WR.fuse(emap, tiles, copy, weights, None, out_w, out_w // 2, zr), abcd
