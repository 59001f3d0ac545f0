"""CPU checks of the disparity-registration restatement (tests/disp_ref.py), which the GPU tests
(tests/test_gpu_disp.py) hold csrc/pf_disp.hip to bit for bit."""
import math

import numpy as np
import pytest

import disp_ref as R

NS = 2409  # samples of a C1 tile's registration grid


@pytest.mark.parametrize("seed", range(10))
def test_planted_recovery(seed):
    """Exact data Y = 1/(a* X + b*) + d* from (1, 1, 1): each parameter to 1e-6 relative."""
    rng = np.random.default_rng(4100 + seed)
    xs = rng.uniform(1e-4, 1 - 1e-4, NS)
    a, b, d = rng.uniform(0.5, 12), rng.uniform(0.8, 3), rng.uniform(-0.1, 0.1)
    ys = 1.0 / (a * xs + b) + d
    coef, s = R.fit(xs, ys)
    print(f"seed {seed}: planted ({a:.6g}, {b:.6g}, {d:.6g}) got {coef} {s}")
    assert coef[2] == 1.0
    for got, want in ((coef[0], a), (coef[1], b), (coef[3], d)):
        assert abs(got - want) <= 1e-6 * abs(want), (got, want)
    assert s["termination"] != "failure" and s["iterations"] < R.MAX_ITER
    assert s["final_cost"] <= s["initial_cost"]


def test_ordered_sum_is_the_documented_order():
    """Lane l adds l, l + 256, ... from 0.0; then p[l] = p[l] + p[l + stride], stride 128 ... 1."""
    rng = np.random.default_rng(7)
    for n in (1, 255, 256, 257, 2409, 5000):
        t = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 8, n)
        part = [0.0] * 256
        for lane in range(256):
            for s in range(lane, n, 256):
                part[lane] = part[lane] + float(t[s])
        stride = 128
        while stride >= 1:
            for lane in range(stride):
                part[lane] = part[lane] + part[lane + stride]
            stride //= 2
        assert R.ordered_sum(t) == part[0]


def test_sums_agree_with_plain_numpy():
    rng = np.random.default_rng(11)
    xs = rng.uniform(1e-4, 1 - 1e-4, NS)
    ys = rng.uniform(1e-4, 1 - 1e-4, NS)
    p = [2.5, 1.25, -0.03]
    S = R.sums(xs, ys, p)
    q = 1.0 / (p[0] * xs + p[1])
    r = q + p[2] - ys
    J = np.stack([-xs * q * q, -q * q, np.ones_like(xs)], 1)
    JtJ = J.T @ J
    want = [0.5 * (r @ r), *(J.T @ r), JtJ[0, 0], JtJ[0, 1], JtJ[0, 2], JtJ[1, 1], JtJ[1, 2],
            JtJ[2, 2]]
    assert np.allclose(S, want, rtol=1e-12, atol=0)
    assert R.cost(xs, ys, p) == S[0]
    # the Jacobian is the derivative of the residual (central differences)
    for k in range(3):
        h = 1e-6
        hi, lo = list(p), list(p)
        hi[k] += h
        lo[k] -= h
        num = (R.cost(xs, ys, hi) - R.cost(xs, ys, lo)) / (2 * h)
        assert abs(num - S[1 + k]) <= 1e-6 * max(1.0, abs(S[1 + k]))


def test_transform_clamps_and_non_finite():
    f = np.float32
    # both X clamps (values at and around the thresholds), interior values
    x = np.array([-1.0, 0.0, 5e-5, f(1e-4), 1e-4 + 1e-6, 0.25, 0.5, 0.75, 1 - 1e-4 - 1e-6,
                  f(1 - 1e-4), 0.99995, 1.0, 7.0], f)
    abcd = np.array([3.0, 1.5, 1.0, -0.05], f)
    y = R.transform(x, abcd)
    xc = np.clip(x.astype(np.float64), 1e-4, 1 - 1e-4)
    want = np.clip(1.0 / (3.0 * xc + 1.5) - 0.05, 0, 1)
    assert np.allclose(y, want, atol=1e-6)
    assert y[0] == y[1] == y[2] and y[-1] == y[-2]  # clamped X give one value each side
    # both Y clamps
    assert R.transform(np.array([0.5], f), np.array([1, 1, 1, 5], f))[0] == 1.0
    assert R.transform(np.array([0.5], f), np.array([1, 1, 1, -5], f))[0] == 0.0
    # a zero denominator: a X + b == 0 exactly at X = 0.5 -> +-inf -> clamps to 1 / 0
    assert R.transform(np.array([0.5], f), np.array([2, -1, 1, 0], f))[0] == 1.0
    assert R.transform(np.array([0.5], f), np.array([2, -1, -1, 0], f))[0] == 0.0
    # 0/0 and a NaN input stay NaN
    assert math.isnan(R.transform(np.array([0.5], f), np.array([2, -1, 0, 0], f))[0])
    assert math.isnan(R.transform(np.array([np.nan], f), abcd)[0])
    assert R.transform(x, abcd).dtype == np.float32


def test_invalid_step_shrinks_radius_and_keeps_parameters():
    """A trial whose cost is not finite is an invalid step: the radius is divided by the
    decrease factor (2, then 4, ...), the parameters stay, and five in a row end the run."""
    rng = np.random.default_rng(3)
    xs = rng.uniform(1e-4, 1 - 1e-4, NS)
    ys = 1.0 / (4.0 * xs + 1.5) + 0.02
    calls = []

    def first_two_fail(p):
        calls.append(tuple(p))
        return [math.inf, math.nan][len(calls) - 1] if len(calls) <= 2 else R.cost(xs, ys, p)

    trace = []
    coef, s = R.fit(xs, ys, trial_cost=first_two_fail, trace=trace)
    assert [t["outcome"] for t in trace[:3]] == ["invalid", "invalid", "accepted"]
    assert [t["radius"] for t in trace[:3]] == [1e4, 5e3, 1.25e3]
    assert trace[0]["x"] == trace[1]["x"] == trace[2]["x"] == (1.0, 1.0, 1.0)
    # and the run still converges to the planted parameters
    ref, _ = R.fit(xs, ys)
    assert np.allclose(coef, ref, rtol=1e-6)
    assert s["termination"] != "failure"

    trace = []
    coef, s = R.fit(xs, ys, trial_cost=lambda p: math.inf, trace=trace)
    assert s["termination"] == "failure" and s["iterations"] == R.MAX_INVALID
    assert len(trace) == R.MAX_INVALID and all(t["outcome"] == "invalid" for t in trace)
    assert [t["radius"] for t in trace] == [1e4, 5e3, 1.25e3, 1.5625e2, 9.765625]
    assert list(coef) == [1.0, 1.0, 1.0, 1.0] and s["x"] == (1.0, 1.0, 1.0)
    assert s["final_cost"] == s["initial_cost"]


def test_non_finite_trial_from_the_model_itself():
    """Without a hook: a sample at which a trial's a X + b is exactly 0 makes its cost infinite."""
    xs = np.array([0.5, 0.25], np.float64)
    ys = np.array([0.5, 0.5], np.float64)
    assert math.isinf(R.cost(xs, ys, [2.0, -1.0, 0.0]))
