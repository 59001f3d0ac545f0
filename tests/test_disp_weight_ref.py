"""CPU checks of the weighted disparity restatement (tests/disp_weight_ref.py), which the GPU tests
(tests/test_gpu_disp_weights.py) hold the library to bit for bit."""
import math

import numpy as np
import pytest

import disp_ref as DR
import disp_weight_cases as CS
import disp_weight_ref as R
import pyoracle as O

f32 = np.float32
NS = 2409  # samples of a C3 tile's registration grid


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("seed", [0, 1])
def test_all_ones_is_the_unweighted_fit(seed):
    """C1: with every weight 1.0f the coefficients and the four LM summary entries are
    disp_ref.fit's bit for bit (1.0 * t is t), the count is the grid's and the sum of w equals it."""
    _, tiles, emap, disp = CS.c1(seed)
    ones = np.ones(disp.size, f32)
    c64, summ = R.register(tiles, disp, ones, emap)
    for p, t in enumerate(tiles):
        xs, ys, _, _ = O.reg_samples(t, np.asarray(disp), np.asarray(emap), CS.ZR)
        want, s = DR.fit(xs, ys)
        assert np.array_equal(_bits(c64[p]), _bits(want)), p
        assert np.array_equal(_bits(summ[p, :4]), _bits(DR.summary_row(s))), p
        assert summ[p, 4] == xs.size == 7865 and summ[p, 5] == xs.size


@pytest.mark.parametrize("seed", range(4))
def test_planted_recovery_with_garbage_under_weight_zero(seed):
    """Exact data on 70 % of the samples under weights in [0.1, 1], garbage (NaN among it) under
    weight 0 on the rest: each parameter to 1e-6 relative, test_disp_ref.py's bar."""
    rng = np.random.default_rng(5200 + seed)
    xs = rng.uniform(1e-4, 1 - 1e-4, NS)
    a, b, d = rng.uniform(0.5, 12), rng.uniform(0.8, 3), rng.uniform(-0.1, 0.1)
    ys = 1.0 / (a * xs + b) + d
    bad = rng.random(NS) < 0.3
    ys[bad] = rng.uniform(1e-4, 1 - 1e-4, int(bad.sum()))
    xs[bad] = np.where(rng.random(int(bad.sum())) < 0.2, np.nan, 1e-4)  # "sky", and NaN
    W = np.where(bad, 0.0, rng.uniform(0.1, 1.0, NS).astype(f32).astype(np.float64))
    coef, s = R.fit(xs, ys, W, W > 0)
    print(f"seed {seed}: planted ({a:.6g}, {b:.6g}, {d:.6g}) got {coef} {s}")
    assert coef[2] == 1.0 and s["used"] == NS - bad.sum()
    for got, want in ((coef[0], a), (coef[1], b), (coef[3], d)):
        assert abs(got - want) <= 1e-6 * abs(want), (got, want)
    assert s["termination"] != "failure" and s["final_cost"] <= s["initial_cost"]
    # the garbage matters: the unweighted fit of the finite part misses the planted parameters
    fin = np.isfinite(xs)
    plain, _ = DR.fit(xs[fin], ys[fin])
    assert abs(plain[0] - a) > 1e-3 * a


def test_zero_one_weights_are_the_fit_on_the_kept_samples():
    """Weights in {0, 1} that drop whole rows of 256 samples: the kept samples, re-laid in order,
    keep their lanes (sample 256 r + l goes to 256 r' + l; the partly filled last row stays last),
    and a dropped row adds +0.0 to every lane, so the lane sums and the tree are those of
    disp_ref.fit on the kept samples alone: bit for bit."""
    rng = np.random.default_rng(77)
    xs = rng.uniform(1e-4, 1 - 1e-4, NS)
    ys = 1.0 / (3.0 * xs + 1.5) + 0.02 + rng.normal(0, 0.01, NS)
    rows = np.arange(NS) // 256
    keep = ~np.isin(rows, (1, 4, 5))
    garbage = xs.copy()
    garbage[~keep] = np.nan
    coef, s = R.fit(garbage, ys, keep.astype(np.float64), keep)
    want, ws = DR.fit(xs[keep], ys[keep])
    assert np.array_equal(_bits(coef), _bits(want))
    assert np.array_equal(_bits(R.summary_row(s)[:4]), _bits(DR.summary_row(ws)))
    assert s["used"] == keep.sum() == s["sum_w"]


def test_scattered_zero_one_weights_agree_with_the_kept_fit():
    """Scattered zeros move the kept samples to other lanes when they are re-laid, so the sums are
    the same numbers added in another order: each differs by a few n eps relative (n = 2,409,
    about 5e-13), the LM's path is the same, and the parameters agree to 1e-12 relative only up to
    the conditioning of the 3 x 3 system; 1e-9 here would be safe, 1e-12 holds for this data
    because the fit is well conditioned (the planted curve with 1 % noise)."""
    rng = np.random.default_rng(78)
    xs = rng.uniform(1e-4, 1 - 1e-4, NS)
    ys = 1.0 / (3.0 * xs + 1.5) + 0.02 + rng.normal(0, 0.01, NS)
    keep = rng.random(NS) < 0.6
    coef, s = R.fit(xs, ys, keep.astype(np.float64), keep)
    want, _ = DR.fit(xs[keep], ys[keep])
    assert s["used"] == keep.sum()
    for k in (0, 1, 3):
        assert abs(coef[k] - want[k]) <= 1e-12 * abs(want[k]) + 1e-12 * abs(want[1]), k


def test_weights_scale_nothing_but_matter():
    """A constant weight scales every sum, not the minimiser: same parameters to 1e-9; a
    non-constant one moves them."""
    rng = np.random.default_rng(79)
    xs = rng.uniform(1e-4, 1 - 1e-4, NS)
    ys = 1.0 / (3.0 * xs + 1.5) + 0.02 + rng.normal(0, 0.01, NS)
    used = np.ones(NS, bool)
    one, _ = R.fit(xs, ys, np.ones(NS), used)
    half, s = R.fit(xs, ys, np.full(NS, 0.5), used)
    assert np.allclose(one, half, rtol=1e-6) and s["sum_w"] == 0.5 * NS
    ramp, _ = R.fit(xs, ys, 0.05 + xs, used)
    assert not np.allclose(one, ramp, rtol=1e-6)


@pytest.mark.parametrize("n_used", [0, 2, 3])
def test_too_few_used_samples(n_used):
    rng = np.random.default_rng(80)
    xs = rng.uniform(1e-4, 1 - 1e-4, NS)
    ys = 1.0 / (3.0 * xs + 1.5) + 0.02
    used = np.zeros(NS, bool)
    used[[5, 700, 2400][:n_used]] = True
    coef, s = R.fit(xs, ys, used * 0.25, used)
    assert s["used"] == n_used and s["sum_w"] == 0.25 * n_used
    if n_used < 3:
        assert np.isnan(coef).all() and s["termination_code"] == 5 and s["iterations"] == 0
        assert math.isnan(s["initial_cost"]) and math.isnan(s["final_cost"])
    else:
        assert np.isfinite(coef).all() and coef[2] == 1.0


def test_range_weights():
    d = np.array([[0.0, 0.5, np.nan, 1.0, -1.0, np.inf, 1e-30, 0.25, 0.75]], f32)
    assert list(R.range_weights(d, 0.0, np.inf)[0]) == [0, 1, 0, 1, 0, 0, 1, 1, 1]
    assert list(R.range_weights(d, 0.0, 1.0)[0]) == [0, 1, 0, 0, 0, 0, 1, 1, 1]
    assert list(R.range_weights(d, 0.0, np.inf, channels=3)[0]) == [0, 0, 0, 1, 0, 0, 1, 0, 0]


def test_range_weights_unbend_the_sky():
    """C1 with the top of every tile at disparity 0: range weights switch those samples off and
    the fitted curves lie closer to the clean tiles' than the unweighted fit's, which the cluster
    at X = 1e-4 bends."""
    _, tiles, emap, disp = CS.c1(0)
    skyd = CS.sky(tiles, disp)
    w = R.range_weights(skyd, 0.0, np.inf)
    clean, _ = R.register(tiles, disp, np.ones(disp.size, f32), emap)
    bent, _ = R.register(tiles, skyd, np.ones(disp.size, f32), emap)
    fixed, summ = R.register(tiles, skyd, w, emap)
    assert (summ[:, 4] >= 3).all() and (summ[:, 4] < 7865).all()
    assert np.isfinite(fixed).all()
    x = np.linspace(0.05, 0.95, 19)

    def curve(c):
        return 1.0 / (c[:, 0:1] * x + c[:, 1:2]) + c[:, 3:4]

    err_fixed = np.abs(curve(fixed) - curve(clean)).max()
    err_bent = np.abs(curve(bent) - curve(clean)).max()
    print(f"curve error vs clean: range weights {err_fixed:.3g}, unweighted {err_bent:.3g}")
    assert err_fixed < err_bent
