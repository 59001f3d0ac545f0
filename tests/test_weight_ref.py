"""tests/weight_ref.py against the oracle and tests/mask_ref.py (CPU only): the restatement that
serves as the reference of the per-pixel tile weights is the oracle's merge where every weight is
1.0f and mask_ref's masked registration and fusion where the weights are in {0, 1}, bit for bit."""

import numpy as np
import pytest

import mask_ref as M
import pyoracle as O
import weight_ref as WR
from test_oracle import GOLDEN

f32 = np.float32


def zero_one(name):
    """(weights in {0, 1}, tile data with NaN under the zeros) for the C1 holes HOLES[name]."""
    _, tiles, _, data = M.c1_inputs()
    w = M.with_holes(np.ones(data.size, f32), name, value=0.0)
    return w, M.with_holes(data, name)


def test_ones_is_the_oracles_merge():
    """wmin * Lp is Lp, ws is the float count, acc * (1 / 1) is acc: out_u16 and abcd of the
    golden C1 merge, and of O.merge."""
    g = np.load(GOLDEN)
    tiles, emap, data = WR.golden_inputs()
    out, abcd = WR.merge(emap, tiles, data, np.ones(data.size, f32))
    assert np.array_equal(abcd.view(np.uint32), g["abcd"].view(np.uint32))
    assert np.array_equal(out, g["out_u16"])
    # and on the synthetic C1 inputs of the other tests
    _, tiles, emap, data = M.c1_inputs()
    out, abcd = WR.merge(emap, tiles, data, np.ones(data.size, f32))
    ref, ref_abcd = O.merge(emap, tiles, np.array(data), M.OUT_W, M.ZR)
    assert np.array_equal(out, ref)
    assert np.array_equal(abcd.view(np.uint32), ref_abcd.view(np.uint32))


@pytest.mark.parametrize("name", ["rect", "tile", "pixel"])
def test_zero_one_weights_are_the_validity_rule(name):
    _, tiles, emap, data = M.c1_inputs()
    w, holed = zero_one(name)
    # registration: mask_ref's sums, counts and coefficients
    c64, summ, sums = WR.register(tiles, holed, w, emap)
    ref64, ref_sums, ref_cnt = M.register(tiles, holed, emap)
    assert np.array_equal(sums[:, :15].view(np.uint64), ref_sums.view(np.uint64))
    assert np.array_equal(summ[:, 0], ref_cnt) and np.array_equal(summ[:, 1], ref_cnt)
    assert np.array_equal(c64.view(np.uint64), ref64.view(np.uint64))
    # fusion under the unmasked coefficients: mask_ref's masked fusion
    ref, stats = M.c1_masked(name)
    got = WR.fuse(emap, tiles, holed, w, M.c1_abcd())
    assert np.array_equal(got, ref)
    # and with the hole's values left in place (weight 0 alone switches the pixels off)
    assert np.array_equal(WR.fuse(emap, tiles, data, w, M.c1_abcd()), ref)


def test_weights_change_the_result_smoothly():
    """The tent is a real weighting: it moves the targets where two tiles overlap, and only
    there (a pixel with one contributing tile gets wmin * Lp * (1 / wmin))."""
    _, tiles, emap, data = M.c1_inputs()
    lv = O.level_dims(M.OUT_W, M.OUT_H, M.ZR, 2)
    d = np.ascontiguousarray(M.transform(tiles, data, M.c1_abcd()))
    ones, _ = WR.weighted_targets(tiles, d, np.ones(d.size, f32), lv)
    tent, ws = WR.weighted_targets(tiles, d, WR.tent(tiles), lv)
    _, _, cover = M.masked_targets(tiles, d, lv)
    both = ~np.isnan(ones)
    assert np.array_equal(np.isnan(tent), np.isnan(ones))
    assert (tent[both & (cover == 2)] != ones[both & (cover == 2)]).any()
    one = both & (cover == 1)
    assert np.allclose(tent[one], ones[one], rtol=4 * np.finfo(f32).eps, atol=0)
    assert (ws[both] > 0).all() and (ws[both] <= 2).all()


class _T:
    def __init__(self, w, h, c=1, offset=0):
        self.width, self.height, self.channels, self.offset = w, h, c, offset


def test_tent_by_hand():
    # 5 x 4: m = (4 + 1) // 2 = 2; t = distance to the nearest edge, counted from 1
    t54 = WR.tent([_T(5, 4)]).reshape(4, 5)
    assert np.array_equal(t54, np.array([[.5, .5, .5, .5, .5],
                                         [.5, 1., 1., 1., .5],
                                         [.5, 1., 1., 1., .5],
                                         [.5, .5, .5, .5, .5]], f32))
    # 6 x 6: m = 3
    a, b = f32(1) / f32(3), f32(2) / f32(3)
    row = {1: [a] * 6, 2: [a, b, b, b, b, a], 3: [a, b, 1, 1, b, a]}
    want = np.array([row[1], row[2], row[3], row[3], row[2], row[1]], f32)
    assert np.array_equal(WR.tent([_T(6, 6)]).reshape(6, 6), want)
    # channels: channel 0 only, and the second tile starts at its offset
    two = WR.tent([_T(5, 4, 3, 0), _T(6, 6, 3, 60)])
    assert two.size == 60 + 108
    assert np.array_equal(two[0:60:3].reshape(4, 5), t54) and not two[1::3].any()
    assert np.array_equal(two[60::3].reshape(6, 6), want) and not two[2::3].any()


def test_usable_weight():
    w = np.array([1.0, 0.5, 0.0, -0.0, -1.0, np.nan, np.inf, -np.inf, 1e-45, 3e38], f32)
    assert np.array_equal(WR.usable(w), np.array([1.0, 0.5, 0, 0, 0, 0, 0, 0, 1e-45, 3e38], f32))
