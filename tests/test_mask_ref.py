"""tests/mask_ref.py against the oracle (CPU only): the compositions that serve as the reference of
the tile-pixel validity rule are the oracle itself wherever no pixel is invalid, bit for bit, and
behave as the rule says where some are."""
import numpy as np

import mask_ref as M
import pyoracle as O
import stitch_ref as SR


def test_composition_is_the_oracle_without_invalid_pixels():
    """Per-tile targets added in tile order + normalize + seed / upsample + jacobi + quantize is
    pfo_solve_depth_all: the proof that the composition is the reference."""
    _, tiles, emap, data = M.c1_inputs()
    ref, _ = O.merge(emap, tiles, np.array(data), M.OUT_W, M.ZR)
    got, stats = M.c1_masked("none")
    assert np.array_equal(got, ref)
    # the condition of exactness, at C1 on all three levels
    assert [s["max_cover"] for s in stats] == [2, 2, 2]
    assert all(s["dropped"] == 0 and s["unwindowed"] == 0 for s in stats)


def test_restated_sums_are_the_oracles_registration():
    """Lane l adds samples l, l + 256, ... from 0.0, then the halving tree: the restated sums give
    O.register_tile's coefficients bit for bit on unmasked tiles."""
    _, tiles, emap, data = M.c1_inputs()
    c64, _, cnt = M.register(tiles, data, emap)
    for p in range(len(tiles)):
        ref64, ref32, deg = O.register_tile(tiles[p], np.array(data), emap, M.ZR, solver="lm")
        assert deg == 3
        assert np.array_equal(c64[p].view(np.uint64), ref64.view(np.uint64)), p
        assert np.array_equal(c64[p].astype(np.float32).view(np.uint32), ref32.view(np.uint32)), p
        assert cnt[p] == O.reg_samples(tiles[p], np.array(data), emap, M.ZR)[0].size


def test_skipped_samples_and_empty_tiles():
    _, tiles, emap, data = M.c1_inputs()
    holed = M.with_holes(M.with_holes(data, "rect"), "tile")
    c64, sums, cnt = M.register(tiles, holed, emap)
    clean, _, full = M.register(tiles, data, emap)
    assert 4 <= cnt[0] < full[0], "the rectangle must drop some of tile 0's samples, not all"
    assert sums[0][9] == cnt[0]
    assert np.isfinite(c64[0]).all() and not np.array_equal(c64[0], clean[0])
    assert cnt[M.ALL_TILE] == 0 and np.isnan(c64[M.ALL_TILE]).all()
    for p in (1, 2, 3, 5):
        assert np.array_equal(c64[p].view(np.uint64), clean[p].view(np.uint64))


def test_masked_fusion_survives_the_holes():
    """A NaN hole read as depth leaves the band at 0; skipped, the panorama stays close to the
    unmasked one, the hole crosses a two-tile seam and leaves pixels un-windowed."""
    _, tiles, emap, data = M.c1_inputs()
    clean, _ = M.c1_masked("none")
    got, stats = M.c1_masked("rect")
    for s in stats:
        assert s["dropped"] > 0 and s["unwindowed"] > 0, stats
    lv = O.level_dims(M.OUT_W, M.OUT_H, M.ZR, 2)
    band = slice(lv.h0, lv.h1 + 1)
    poisoned, _ = O.solve_depth_all(emap, tiles, M.transform(tiles, M.with_holes(data, "rect"),
                                                             M.c1_abcd()), M.OUT_W, M.ZR)
    assert (poisoned[band] == 0).mean() > 0.9
    assert (got[band] == 0).mean() < 0.01
    diff = np.abs(got[band].astype(np.int64) - clean[band].astype(np.int64))
    assert 0 < diff.mean() < 655  # under 1 % of full scale on average; the hole does change it


def test_stitch_valid_without_invalid_pixels_is_the_stitch():
    _, tiles, _, data = M.c1_inputs()
    abcd = M.c1_abcd()
    assert np.array_equal(M.stitch_valid(tiles, data, 256, 128), SR.stitch(tiles, data, 256, 128))
    assert np.array_equal(M.stitch_valid(tiles, data, 256, 128, abcd),
                          SR.stitch(tiles, data, 256, 128, abcd))
    holed = M.with_holes(data, "tile")
    got = M.stitch_valid(tiles, holed, 256, 128)
    _, first = SR.cover(tiles, 256, 128)
    count, _ = SR.cover(tiles, 256, 128)
    only4 = (first == M.ALL_TILE) & (count == 1)
    assert only4.any() and (got[only4] == 0).all()
