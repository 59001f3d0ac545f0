"""tests/mask_shapes.py on the CPU: the case table of tests/test_gpu_mask_shapes.py, and the proof
that the reference is a reference at every case.

* the rows come from test_fuse_shapes.SHAPES and take, under the rule, the engines restated there
  with the certificate forced false;
* every hole set does what it is for, read from masked_fuse's stats at that size (a case that
  does not is a wrong case: the hole moves, the assertion stays);
* with no hole the composition is pfo_solve_depth_all bit for bit, at every row and layout, and
  mask_ref.register / stitch_valid are the oracle's unmasked registration and stitch.

Every layout here covers a pixel at most twice (asserted), so the composition's sum is order-free
and proven against the oracle everywhere; mask_shapes.cover_limit() would lift the condition for a
layout that covers more, and the sum would there restate targets_patch's ascending order instead.
"""
import numpy as np
import pytest

import mask_ref as M
import mask_shapes as MS
import pyoracle as O
import stitch_ref as SR
import test_fuse_shapes as TS

ZR = M.ZR
SIZE_IDS = [MS.size_id(s) for s in MS.SIZES]


# ---- a. the rows --------------------------------------------------------------------------------
def test_rows_come_from_the_shape_table():
    assert [(r[0], r[1]) for r in MS.ROWS] == sorted(MS.SIZES, key=MS.ROW_INDEX.get)
    assert len(MS.ROWS) == len(MS.SIZES) == 7
    for r in MS.ROWS:
        assert r in TS.SHAPES
        ew, eh, ec = TS.BASELINES[MS.ROW_INDEX[(r[0], r[1])] % len(TS.BASELINES)]
        e = MS.row_case((r[0], r[1])).emap
        assert e.shape == ((eh, ew) if ec == 1 else (eh, ew, ec))


@pytest.mark.parametrize("size", MS.SIZES, ids=SIZE_IDS)
def test_engines_under_the_rule(size):
    """No certificate under the rule: sweeps where tcap < 1, otherwise the general streamed
    passes; the rows that are resident by default are streamed here."""
    case = MS.row_case(size)
    got = MS.expected_engines(case)
    default = TS.SHAPES[MS.ROW_INDEX[size]][3]
    for level, engine in enumerate(got):
        lv = case.level(level)
        assert engine == ("sweeps" if TS.tcap(lv) < 1 else "streamed"), level
        assert engine == ("streamed" if default[level] == "resident" else default[level]), level
    want0 = "sweeps" if size in ((500, 248), (440, 220)) else "streamed"
    assert got == [want0, "streamed", "streamed"]
    if size in ((1024, 400), (2048, 400)):
        assert default[0] == "resident"
    if size == (1024, 400):
        assert default[1] == "resident"


def test_rows_reach_what_they_name():
    lv = {s: [MS.row_case(s).level(k) for k in range(3)] for s in MS.SIZES}
    assert lv[(600, 300)][0].w % 4 == 2 and lv[(600, 300)][0].h % 2 == 1
    assert all(L.w % 64 for L in lv[(600, 300)])  # partial patches on every level
    # ragged last strips, whichever strip width a pass takes, on the finest level
    assert all(lv[(600, 300)][2].w % V for V in M.STRIP_WIDTHS if V != 120)
    assert lv[(496, 248)][0].w == 124  # a strip (128 virtual columns) wider than the row
    assert lv[(500, 248)][0].w % 2 == 1 and lv[(440, 220)][0].w < 124
    assert lv[(1096, 500)][2].h != lv[(1096, 500)][2].w // 2
    assert lv[(1024, 400)][0].w == 256 and lv[(1024, 400)][1].w == 512
    assert lv[(2048, 400)][0].w == 512


# ---- b, c. the hole sets land where they are meant to -------------------------------------------
def _check_placement(case, name, stats):
    fin = stats[-1]
    if name == "seam":
        assert all(s["dropped"] > 0 and s["unwindowed"] > 0 for s in stats), stats
    elif name == "bandrows":
        # every level whose row h1-1 the layout covers at all (level 0 of 440x220 does not: its
        # tiles' boxes end at h1-2); the two finer levels always
        for level, s in enumerate(stats):
            lv = case.level(level)
            cov = MS.cover(case, level)
            assert s["unwindowed_first_row"] > 0, (level, s)
            if cov[lv.h1 - 1].any() or level > 0:
                assert s["unwindowed_last_row"] > 0, (level, s)
    elif name == "edgecols":
        assert all(s["unwindowed_first_col"] > 0 and s["unwindowed_last_col"] > 0
                   for s in stats), stats
    elif name == "checker":
        # the finest level: two or more 64 x 8 patches, and either side of the first strip border
        # whichever of the five strip widths a pass takes
        assert fin["unwindowed_patches"] >= 2, fin
        assert fin["strip_seams"] == list(M.STRIP_WIDTHS), fin
        lv = case.level(case.nlevels - 1)
        x0, nx, ny = MS.CHECKER
        assert nx >= 70 and ny >= 12 and x0 < 128 < x0 + nx and x0 + nx <= lv.w
    elif name == "isolated":
        assert stats[MS.isolated_level(case)]["isolated"] > 0, stats
        assert stats[MS.isolated_level(case)]["unwindowed"] > 100, stats
    elif name == "tile":
        assert all(s["dropped"] > 0 and s["unwindowed"] > 0 for s in stats), stats
    assert all(s["max_cover"] <= 2 for s in stats)


@pytest.mark.parametrize("name", MS.SETS)
@pytest.mark.parametrize("size", MS.SIZES, ids=SIZE_IDS)
def test_hole_set_placement(size, name):
    case = MS.row_case(size)
    stats = MS.stats(case, name)
    print(f"\n{case.name} {name}: dropped / un-windowed per level "
          + " ".join(f"{s['dropped']}/{s['unwindowed']}" for s in stats))
    _check_placement(case, name, stats)
    d = MS.raw(case, name)
    assert np.isnan(d).any() and not np.isnan(case.data).any()


@pytest.mark.parametrize("size", MS.FULL_CHECKS, ids=MS.size_id)
def test_composition_stats_are_the_placement_stats(size):
    """masked_fuse records the same stats as the solve-free masked_stats."""
    case = MS.row_case(size)
    for name in ("seam", "checker"):
        assert MS.composition(case, name)[1] == MS.stats(case, name)


# ---- d. the other layouts -----------------------------------------------------------------------
@pytest.mark.parametrize("layout", MS.LAYOUTS)
def test_layout_cover_and_hole_sets(layout):
    case = MS.layout_case(layout)
    assert MS.max_cover(case) == 2 and MS.cover_limit(case) == 2
    for name in MS.SETS:
        _check_placement(case, name, MS.stats(case, name))


@pytest.mark.parametrize("layout,count", [("LERES", 1), ("MIDAS", 44), ("LERES3", 1),
                                          ("MIDAS3", 44)])
def test_a_clamped_tap_reads_an_invalid_pixel(layout, count):
    """Level 0 of LeReS 64x48 has 1 clamped tap and MiDaS 40x30 has 44 (the oracle's own count);
    the `clamped` hole is the element one of them lands on, and the stencil that reads it through
    the clamp loses its tile."""
    case = MS.layout_case(layout)
    lv = case.level(0)
    _, _, _, oob = O.targets(case.tiles, np.array(case.data), lv)
    maps = MS.tile_maps(case, 0)
    assert oob == count == sum(int(m[2].sum()) for m in maps)
    (p, el), = MS.holes(case, "clamped")
    inbox, taps, clamped = maps[p]
    t = case.tiles[p]
    assert el.size == 1 and el[0] in (0, (t.width * t.height - 1) * t.channels)
    hit = (clamped & (taps == el[0])).any(-1)  # the pixels that read the hole through the clamp
    assert hit.any()
    s, c = O.targets_subset(case.tiles, p, p + 1, MS.raw(case, "clamped"), lv)
    band = MS._band(lv)
    assert np.isnan(s[hit & band]).all() and (c[hit & band] == 1).all()
    stats = MS.stats(case, "clamped")
    assert stats[0]["dropped"] + stats[0]["unwindowed"] > 0


# ---- e. the proof -------------------------------------------------------------------------------
@pytest.mark.parametrize("size", MS.SIZES, ids=SIZE_IDS)
def test_composition_is_the_oracle_at_every_row(size):
    case = MS.row_case(size)
    got, stats = MS.composition(case, "none")
    d = M.transform(case.tiles, case.data, MS.abcd(case))
    ref, oops = O.solve_depth_all(case.emap, case.tiles, d, case.out_w, ZR, out_h=case.out_h)
    assert oops == 0 and ref.shape == (case.out_h, case.out_w)
    assert np.array_equal(got, ref)
    assert all(s["dropped"] == 0 and s["unwindowed"] == 0 and s["isolated"] == 0 for s in stats)
    assert [s["max_cover"] for s in stats] == [2, 2, 2]
    assert np.count_nonzero(ref) > 0


@pytest.mark.parametrize("layout", MS.LAYOUTS)
def test_composition_is_the_oracle_at_every_layout(layout):
    case = MS.layout_case(layout)
    got, stats = MS.composition(case, "none")
    ref, abcd = O.merge(case.emap, case.tiles, np.array(case.data), case.out_w, ZR)
    assert np.array_equal(abcd, MS.abcd(case))
    assert np.array_equal(got, ref)
    assert all(s["dropped"] == 0 and s["unwindowed"] == 0 for s in stats)


@pytest.mark.parametrize("layout", ["MIXED", "LERES3", "MIDAS3"])
def test_register_is_the_oracle_at_the_layouts(layout):
    """The restated sums give O.register_tile's coefficients on unmasked tiles of mixed sizes and
    of three channels; the registration holes leave 0, exactly 3 and exactly 4 valid samples."""
    case = MS.layout_case(layout)
    c64, _, cnt = M.register(case.tiles, case.data, case.emap)
    for p, t in enumerate(case.tiles):
        ref64, ref32, deg = O.register_tile(t, np.array(case.data), case.emap, ZR, solver="lm")
        assert deg == 3
        assert np.array_equal(c64[p].view(np.uint64), ref64.view(np.uint64)), p
        assert np.array_equal(c64[p].astype(np.float32).view(np.uint32), ref32.view(np.uint32)), p
    d = M.apply_holes(case.tiles, case.data, MS.reg_holes(case))
    h64, sums, hcnt = M.register(case.tiles, d, case.emap)
    e, three, four = (MS.REG_TILES[k] for k in ("empty", "three", "four"))
    assert (hcnt[e], hcnt[three], hcnt[four]) == (0, 3, 4)
    assert np.isnan(h64[e]).all() and np.isnan(h64[three]).all()
    want, _ = O.lm_moments(sums[four])
    if not np.isfinite(want).all():
        want = np.full(4, np.nan)
    assert np.array_equal(h64[four], want, equal_nan=True)
    if case.channels == 3:
        import tile_shapes as TL
        assert TL.fill_kept(np.where(np.isnan(d), TL.FILL, d)), "a hole left channel 0"
        assert not np.isnan(TL.channel(d, 1)).any() and not np.isnan(TL.channel(d, 2)).any()


STITCH_CASES = [("600x300", s) for s in MS.STITCH_SIZES] + [("LERES", (512, 256)),
                                                            ("LERES3", (512, 256)),
                                                            ("MIDAS3", (512, 256))]


def _stitch_case(name):
    return MS.row_case((600, 300)) if name == "600x300" else MS.layout_case(name)


@pytest.mark.parametrize("name,size", STITCH_CASES, ids=lambda v: v if isinstance(v, str)
                         else MS.size_id(v))
def test_stitch_valid_is_the_stitch_and_picks_the_third_tile(name, size):
    case = _stitch_case(name)
    W, H = size
    cf = MS.abcd(case)
    assert np.array_equal(M.stitch_valid(case.tiles, case.data, W, H),
                          SR.stitch(case.tiles, case.data, W, H))
    assert np.array_equal(M.stitch_valid(case.tiles, case.data, W, H, cf),
                          SR.stitch(case.tiles, case.data, W, H, cf))
    holes, third = MS.stitch_holes(case.tiles, W, H)
    assert third is not None, "every layout here has a pixel inside three boxes"
    d = M.apply_holes(case.tiles, case.data, holes)
    y, x, p = third
    ins, els = MS.stitch_maps(case.tiles, W, H)
    cand = np.flatnonzero(ins[:, y, x])
    assert cand[2] == p and all(np.isnan(d[case.tiles[q].offset + els[q, y, x]])
                                for q in cand[:2])
    v = d[case.tiles[p].offset + els[p, y, x]]
    assert not np.isnan(v)
    got = M.stitch_valid(case.tiles, d, W, H)
    assert got[y, x] == SR.quantize(np.array([v]))[0]  # the pick: the third candidate's value
    assert not np.array_equal(got, SR.stitch(case.tiles, case.data, W, H))
