"""CPU checks of the robust-registration restatement (tests/robust_ref.py), which the GPU tests
(tests/test_gpu_robust.py) hold csrc/pf_robust.hip and the loss instantiation of csrc/pf_disp.hip
to bit for bit."""
import math
import os

import numpy as np
import pytest

import disp_ref as DR
import fusion_ref as FR
import pyoracle as O
import robust_ref as R

NS = 2409  # samples of a C1 tile's registration grid


def _scene_like(seed, n=NS):
    """Samples of a smooth response with small noise: every residual of the fit stays far
    inside a = 10, and at the start (1,1,1,1) too (|r| < 4)."""
    rng = np.random.default_rng(900 + seed)
    xs = DR.clamp_samples(rng.uniform(0.05, 0.9, n))
    ys = DR.clamp_samples(0.8 * xs ** 1.2 + 0.05 + rng.normal(0, 0.003, n))
    return xs, ys


@pytest.mark.parametrize("seed", range(3))
def test_matches_the_oracle_when_no_sample_leaves_the_inlier_region(seed):
    """Huber at a = 10: rho = s, rho' = 1 on every sample of every evaluation, so the run is the
    oracle's sample-wise pfo_lm_fit up to the summation order: cost to rtol 1e-12, coefficients to
    ABCD_RTOL, the same iteration count and termination."""
    xs, ys = _scene_like(seed)
    got, s = R.fit(xs, ys, "huber", 10.0)
    want, so = O.lm_fit(xs, ys)
    print(f"seed {seed}: restatement {got} {s}\n  oracle {want} {so}")
    assert s["inliers"] == s["used"] == xs.size
    assert s["iterations"] == so["iterations"] and s["termination"] == so["termination"]
    assert abs(s["initial_cost"] - so["initial_cost"]) <= 1e-12 * so["initial_cost"]
    assert abs(s["final_cost"] - so["final_cost"]) <= 1e-12 * so["final_cost"]
    assert FR.rel_diff(got, want).max() <= FR.ABCD_RTOL
    # and with no loss at all the restatement takes the same steps bit for bit
    plain, sp = R.fit(xs, ys, None)
    assert np.array_equal(plain, got) and sp["final_cost"] == s["final_cost"]


@pytest.mark.parametrize("kind", ["huber", "softl1"])
def test_loss_formulas(kind):
    """rho(0) = 0, rho' is the derivative of rho (central differences), rho' in (0, 1],
    non-increasing (rho'' <= 0: Corrector's first branch), and Huber's two branches meet at b."""
    a = 0.02
    s = np.concatenate([np.linspace(1e-7, 4 * a * a, 400), np.geomspace(4 * a * a, 1.0, 200)])
    rho0, rho1 = R.loss(kind, a, s)
    h = 1e-9
    up, _ = R.loss(kind, a, s + h)
    dn, _ = R.loss(kind, a, s - h)
    num = (up - dn) / (2 * h)
    # Huber's derivative jumps in slope (not in value) at s = b: skip the two nearest points
    keep = np.abs(s - a * a) > 2 * h
    assert np.max(np.abs(num - rho1)[keep]) <= 1e-5
    assert np.all(rho1 > 0) and np.all(rho1 <= 1.0) and np.all(np.diff(rho1) <= 0)
    z0, z1 = R.loss(kind, a, np.array([0.0]))
    assert z0[0] == 0.0 and z1[0] == 1.0
    if kind == "huber":
        at0, at1 = R.loss(kind, a, np.array([a * a]))
        assert at0[0] == a * a and at1[0] == 1.0  # s > b is strict
        up0, up1 = R.loss(kind, a, np.array([np.nextafter(a * a, 1.0)]))
        assert abs(up0[0] - a * a) <= 1e-15 and abs(up1[0] - 1.0) <= 1e-12
    # a huge residual: rho' stays positive (the DBL_MIN floor), rho finite
    big0, big1 = R.loss(kind, a, np.array([1e300]))
    assert math.isfinite(big0[0]) and big1[0] >= R.DBL_MIN
    # kind None is least squares
    n0, n1 = R.loss(None, a, s)
    assert np.array_equal(n0, s) and np.all(n1 == 1.0)


@pytest.mark.parametrize("model", ["cubic", "disparity"])
@pytest.mark.parametrize("kind", ["huber", "softl1"])
def test_sums_are_the_corrected_quantities(kind, model):
    """The sums equal 0.5 sum rho, J_c' r_c and J_c' J_c of the corrected residual and Jacobian
    (plain numpy, rtol 1e-12), and J_c' r_c is the gradient of the cost (central differences)."""
    xs, ys, _ = R.planted_samples(1)
    p = [0.3, -0.4, 1.1, 0.05] if model == "cubic" else [2.5, 1.25, -0.03]
    n = len(p)
    a = 0.02
    S = R.sums(xs, ys, p, kind, a, model)
    assert len(S) == 1 + n + n * (n + 1) // 2
    r, J = R.residual_and_rows(xs, ys, p, model)
    rho0, rho1 = R.loss(kind, a, r * r)
    w = np.sqrt(rho1)
    Jc = np.stack([w * (np.full_like(xs, j) if isinstance(j, float) else j) for j in J], 1)
    JtJ = Jc.T @ Jc
    want = [0.5 * rho0.sum(), *(Jc.T @ (w * r))] + [JtJ[i, j] for i in range(n)
                                                   for j in range(i, n)]
    assert np.allclose(S, want, rtol=1e-12, atol=0)
    assert R.cost(xs, ys, p, kind, a, model) == S[0]
    assert np.count_nonzero(r * r > a * a) > 100  # the loss is active on this input
    for k in range(n):
        h = 1e-7
        hi, lo = list(p), list(p)
        hi[k] += h
        lo[k] -= h
        num = (R.cost(xs, ys, hi, kind, a, model) - R.cost(xs, ys, lo, kind, a, model)) / (2 * h)
        assert abs(num - S[1 + k]) <= 1e-5 * max(1.0, abs(S[1 + k])), (k, num, S[1 + k])


@pytest.mark.parametrize("model", ["cubic", "disparity"])
def test_every_sum_goes_through_ordered_sum(model):
    """All 15 (10) sums of a Jacobian evaluation, the one of a trial, and nothing else."""
    xs, ys, _ = R.planted_samples(2)
    calls = []

    def spy(t):
        calls.append(t.size)
        return DR.ordered_sum(t)

    n = R.MODELS[model]
    nsums = 1 + n + n * (n + 1) // 2
    assert nsums == (15 if model == "cubic" else 10)
    R.sums(xs, ys, [1.0] * n, "huber", 0.02, model, ordered_sum=spy)
    assert calls == [xs.size] * nsums
    calls.clear()
    R.cost(xs, ys, [1.0] * n, "huber", 0.02, model, ordered_sum=spy)
    assert calls == [xs.size]
    calls.clear()
    trace = []
    _, s = R.fit(xs, ys, "huber", 0.02, model, trace=trace, ordered_sum=spy)
    accepted = sum(t["outcome"] == "accepted" for t in trace)
    trials = sum(t["outcome"] != "invalid" for t in trace)
    assert len(calls) == nsums * (1 + accepted) + trials


@pytest.mark.parametrize("seed", R.OUTLIER_SEEDS)
def test_huber_beats_least_squares_on_planted_outliers(seed):
    """10 % of the y values replaced by U(0, 1): Huber at a = 0.02 has max |fit - truth| over
    x in 0.1-0.6 at most one quarter of the least-squares fit's."""
    xs, ys, out = R.planted_samples(seed)
    plain, sp = R.fit(xs, ys, None)
    huber, sh = R.fit(xs, ys, "huber", 0.02)
    soft, ss = R.fit(xs, ys, "softl1", 0.02)
    e0, e1, e2 = R.max_error(plain), R.max_error(huber), R.max_error(soft)
    print(f"seed {seed}: none {e0:.5f} ({sp['iterations']} it)  huber {e1:.5f} "
          f"({sh['iterations']} it, {sh['termination']}, {sh['inliers']} inliers)  "
          f"softl1 {e2:.5f} ({ss['iterations']} it)")
    assert e1 <= 0.25 * e0
    assert e2 <= 0.25 * e0
    # the samples beyond a are, up to the noise tail, the planted ones
    assert abs((xs.size - sh["inliers"]) - int(out.sum())) <= 0.1 * out.sum()
    # the plain fit agrees with the oracle's (same data, another summation order)
    want, _ = O.lm_fit(xs, ys)
    assert np.max(np.abs(R.cubic(plain, R.GRID) - R.cubic(want, R.GRID))) <= 1e-5


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "robust_ref.npz")
# Summary::message's first words per termination of the restatement
MESSAGES = {"function_tolerance": "Function tolerance reached",
            "parameter_tolerance": "Parameter tolerance reached",
            "gradient_tolerance": "Gradient tolerance reached",
            "no_convergence": "Maximum number of iterations reached",
            "min_trust_region_radius": "Minimum trust region radius reached",
            "failure": "Number of successive invalid steps"}
# Ceres appends an iteration to Summary::iterations when the next one begins
# (FinalizeIterationAndCheckIfMinimizerCanContinue), where it also tests the gradient, the
# iteration limit and the radius: a run ended there has recorded its last iteration (and iteration
# 0), one ended inside an iteration by a tolerance or by invalid steps has not.
EXTRA_ENTRY = ("gradient_tolerance", "no_convergence", "min_trust_region_radius")


def _records():
    g = np.load(GOLDEN)
    n = 0
    k = 0
    while f"xs{k}" in g.files:
        for loss in g["losses"]:
            for a in g["scales"]:
                yield g, k, str(loss), float(a), n
                n += 1
        k += 1
    assert n == g["coef"].shape[0] == 32 and k == 8


def test_real_ceres():
    """Every record of tests/golden/robust_ref.npz (real Ceres 1.13 under HuberLoss /
    SoftLOneLoss, tools/make_robust_golden.py): the same termination and iteration count, the
    fitted values at the samples within 1e-5 absolute, the costs to 1e-9 relative, and the
    coefficients within ABCD_RTOL where the tile is well-conditioned (kappa from the inputs)."""
    held = 0
    for g, k, loss, a, n in _records():
        xs, ys, model = g[f"xs{k}"], g[f"ys{k}"], str(g[f"model{k}"])
        c, s = R.fit(xs, ys, loss, a, model)
        ref = g["coef"][n]
        msg = str(g["message"][n])
        assert MESSAGES[s["termination"]] in msg, (k, loss, a, s, msg)
        assert g["entries"][n] == s["iterations"] + (s["termination"] in EXTRA_ENTRY), (k, loss, a)
        assert abs(s["initial_cost"] - g["cost"][n, 0]) <= 1e-9 * g["cost"][n, 0]
        assert abs(s["final_cost"] - g["cost"][n, 1]) <= 1e-9 * g["cost"][n, 1]
        if model == "cubic":
            dv = np.max(np.abs(R.cubic(c, xs) - R.cubic(ref, xs)))
        else:
            dv = np.max(np.abs((1.0 / (c[0] * xs + c[1]) + c[3])
                               - (1.0 / (ref[0] * xs + ref[1]) + ref[3])))
        kappa = FR.kappa(xs)
        rel = FR.rel_diff(c, ref).max()
        print(f"case {k} {model} {loss} a={a}: {s['iterations']} iterations, {s['termination']}, "
              f"max |fit diff| {dv:.3g}, kappa {kappa:.3g}, coefficient rel diff {rel:.3g}")
        assert dv <= 1e-5
        if kappa <= FR.KAPPA_MAX:
            held += 1
            assert rel <= FR.ABCD_RTOL, (k, loss, a, c, ref)
    print(f"{held} of 32 records are well-conditioned")


def test_validity_mask():
    """Skipped samples keep their lanes and add nothing; fewer than 4 left gives NaN, code 5."""
    xs, ys, _ = R.planted_samples(3)
    valid = np.ones(xs.size, bool)
    valid[100:900] = False
    xbad = xs.copy()
    xbad[~valid] = np.nan
    c, s = R.fit(xbad, ys, "huber", 0.02, valid=valid)
    assert s["used"] == xs.size - 800 and np.isfinite(c).all() and s["inliers"] <= s["used"]
    # the same fit as on arrays whose skipped entries hold anything else
    xany = xs.copy()
    xany[~valid] = 0.123
    c2, s2 = R.fit(xany, ys, "huber", 0.02, valid=valid)
    assert np.array_equal(c, c2) and s == s2
    few = np.zeros(xs.size, bool)
    few[[5, 300, 2000]] = True
    c, s = R.fit(xs, ys, "huber", 0.02, valid=few)
    assert np.isnan(c).all() and s["termination_code"] == 5 and s["used"] == 3
    assert s["iterations"] == 0 and s["inliers"] == 0
    row = R.summary_row(s)
    assert row.shape == (6,) and np.isnan(row[0]) and np.isnan(row[1]) and row[4] == 3.0


def test_non_finite_trial_is_an_invalid_step():
    """The disparity model under a loss: a sample at which a trial's a X + b is exactly 0."""
    xs = np.array([0.5, 0.25], np.float64)
    ys = np.array([0.5, 0.5], np.float64)
    assert not math.isfinite(R.cost(xs, ys, [2.0, -1.0, 0.0], "huber", 0.02, "disparity"))
