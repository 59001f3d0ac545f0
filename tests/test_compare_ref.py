"""CPU check of the ErrorCompare restatement (tests/compare_ref.py; Depth.cpp:2460-2634) against
tests/golden/compare_ref.npz: nine small file pairs, each in depth mode and in disparity mode with
several align_way / cap settings, with the seven floats that the reference's own compiled
ErrorCompare returned (printed at %.9g, which round-trips a float32) and the pixels of the shifted
PNG it wrote (tools/make_compare_golden.py).

Bar: the seven metrics equal as float32, the shifted pixels equal.  The restatement calls the CPU
oracle for both ErrorEmap calls and is numpy float32 otherwise, so this pins the oracle's
ErrorEmap to the reference as well -- for depth maps, for a gt disparity that reaches 1e5, and for
given maps clipped at 10."""
import os

import numpy as np
import pytest

import compare_ref as R
import pf_layouts as PL

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "compare_ref.npz")
ZR = PL.ZENITH_RANGE
NRUNS = 54


@pytest.fixture(scope="module")
def cases():
    return R.golden_cases(np.load(GOLDEN))


def _maps(c):
    return R.load_map(c["gt_raw"], c["gt_kind"]), R.load_map(c["given_raw"], c["given_kind"], True)


@pytest.mark.parametrize("k", range(NRUNS))
def test_restatement_matches_reference(cases, k):
    c = cases[k]
    gt, given = _maps(c)
    got = R.compare(gt, given, ZR, c["disp"], c["align_way"], c["cap"])
    mine = np.array([got[m] for m in R.METRICS], np.float32)
    print(c["id"], mine, c["ref"])
    assert np.array_equal(mine.view(np.uint32), c["ref"].view(np.uint32)), (c["id"], mine, c["ref"])
    assert got["shifted"].shape == c["pixels"].shape
    assert np.array_equal(got["shifted"], c["pixels"]), c["id"]


def test_golden_covers_the_cases(cases):
    """Every input combination in both modes; in disparity mode o < 0, 5-50 % black pixels in
    every pair and a pixel at the cap in most; the fixture stays small."""
    assert len(cases) == NRUNS
    shapes = {(c["gt_raw"].shape[:2], c["given_raw"].shape[:2]) for c in cases}
    assert shapes == {((32, 64), (32, 64)), ((50, 100), (33, 64)), ((37, 75), (37, 75))}
    given_forms = {(c["given_kind"], c["given_raw"].shape[2:]) for c in cases}
    assert given_forms == {("png16", ()), ("pfm", ()), ("png8", (3,)), ("png8", (2,))}
    assert {(c["gt_kind"], c["gt_raw"].shape[2:]) for c in cases} == {("png16", ()), ("png8", (3,))}
    for pair in range(9):
        runs = [c for c in cases if c["pair"] == pair]
        assert {c["disp"] for c in runs} == {False, True}
        assert len({(c["align_way"], c["cap"]) for c in runs if c["disp"]}) >= 3
    capped = 0
    for c in cases:
        if not (c["disp"] and c["align_way"] == 1 and c["cap"]):
            continue
        r = R.compare(*_maps(c), ZR, True, 1, True)
        black = 1.0 - r["n_nonblack"] / r["depth"].size
        assert r["fit_o"] < 0 and 0.05 < black < 0.5, (c["id"], r["fit_o"], black)
        capped += int((r["depth"] == 10).any())
    assert capped >= 6
    assert os.path.getsize(GOLDEN) < 100 * 1024


def test_conv_repeats_per_channel():
    """conv on a 3-channel map is three inversions, on a 2-channel map two: nearly the identity,
    not bit for bit."""
    v = np.array([0.3, 3.0, 7.0, 1e-6, 0.0, -0.3], np.float32)
    once = R.conv(v, 1)
    assert np.array_equal(once[:3], np.float32(1.0) / v[:3]) and np.array_equal(once[3:5], v[3:5])
    assert np.array_equal(R.conv(v, 3), R.conv(R.conv(once, 1), 1))
    twice = R.conv(np.linspace(0.01, 5, 4001, dtype=np.float32), 2)
    back = np.linspace(0.01, 5, 4001, dtype=np.float32)
    assert np.allclose(twice, back, rtol=3e-7) and not np.array_equal(twice, back)


def test_quantise_rules():
    v = np.array([-1.0, 0.0, 0.5, 1.0, 1.7, np.nan, np.inf, -np.inf, 0.999], np.float32)
    assert R.quantise(v).tolist() == [0, 0, 127, 255, 255, 0, 255, 0, 254]
    assert R.save8bit(v).tolist() == [0, 0, 127, 255, 255, 0, 255, 0, 254]


def test_nan_is_not_black_and_moves_no_bound():
    v = np.array([[0.0, 2.0, np.nan, 5.0, 5e-5]], np.float32)
    vmin, vmax, n, nv = R.normalise(v)
    assert (float(vmin), float(vmax), n) == (2.0, 5.0, 3)
    assert nv[0, 0] == 0 and nv[0, 1] == 0 and np.isnan(nv[0, 2]) and nv[0, 3] == 1
    assert nv[0, 4] == np.float32(5e-5)
    vmin, vmax, n, _ = R.normalise(np.zeros((2, 2), np.float32))
    assert (float(vmin), float(vmax), n) == (R.FLT_MAX, -R.FLT_MAX, 0)
