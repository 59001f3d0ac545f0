"""The CPU restatement of the planar-depth tile path (tests/planar_ref.py) proved on the CPU:

* with an all-ones factor its sums and fits are mask_ref.reg_sums, the oracle's registration,
  disp_ref.fit and the robust restatement, bit for bit, and its apply is the oracle's transform;
* the factor agrees with |corner0 + x hedge + y vedge| of the oracle's fp32 tile geometry;
* the value of the feature at C1: planar tiles fused with the factor are as close to the ground
  truth as ray tiles are today, and planar tiles read as ray distance are at least twice as far.
"""
import functools

import numpy as np
import pytest

import disp_ref as DR
import mask_ref as M
import pf_layouts as PL
import pf_synth
import planar_ref as P
import pyoracle as O
import robust_ref as RR

ZR = PL.ZENITH_RANGE
f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _c1_samples(p):
    _, tiles, emap, data = M.c1_inputs()
    xs, ys, _, _ = O.reg_samples(tiles[p], np.array(data), emap, ZR)
    return xs, ys


# ---- an all-ones factor is today's arithmetic ---------------------------------------------------
@pytest.mark.parametrize("p", [0, 4])
def test_unit_factor_moment_sums_and_solves(p):
    _, tiles, emap, data = M.c1_inputs()
    xs, ys = _c1_samples(p)
    one = np.ones_like(xs)
    S = P.reg_sums(xs, ys, one)
    assert np.array_equal(_bits(S[:15]), _bits(M.reg_sums(xs, ys)))
    assert S[15] == xs.size == S[9]
    valid = np.arange(xs.size) % 3 != 0
    Sv = P.reg_sums(xs, ys, one, valid)
    assert np.array_equal(_bits(Sv[:15]), _bits(M.reg_sums(xs, ys, valid)))
    assert Sv[15] == np.count_nonzero(valid)
    # the solves: the oracle's registration of the same tile, both solvers and degree 1
    for degree, solver in ((3, "lm"), (3, "normal"), (1, "normal")):
        want, _, _ = O.register_tile(tiles[p], np.array(data), emap, ZR, degree, solver)
        got, _ = P.register(xs, ys, one, None, degree, solver)
        assert np.array_equal(_bits(got), _bits(want)), (degree, solver)


def test_unit_factor_sample_wise_fits():
    xs, ys = _c1_samples(1)
    one = np.ones_like(xs)
    # the disparity model on disparity-like x
    xd = DR.clamp_samples(1.0 - xs)
    want, ws = DR.fit(xd, ys)
    got, gs = P.fit(xd, ys, one, None, 0.0, "disparity")
    assert np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(_bits(DR.summary_row(gs)), _bits(DR.summary_row(ws)))
    valid = np.arange(xs.size) % 5 != 0
    for model, x in (("cubic", xs), ("disparity", xd)):
        for kind in ("huber", "softl1"):
            v = valid if model == "cubic" else None
            want, ws = RR.fit(x, ys, kind, 0.02, model, valid=v)
            got, gs = P.fit(x, ys, one, kind, 0.02, model, valid=v)
            assert np.array_equal(_bits(got), _bits(want)), (model, kind)
            assert np.array_equal(_bits(RR.summary_row(gs)), _bits(RR.summary_row(ws)))


def test_unit_factor_apply_is_the_oracles_transform():
    _, tiles, _, data = M.c1_inputs()
    abcd = M.c1_abcd()
    d = M.with_holes(data, "rect")  # NaN stays NaN
    ones = [np.ones((t.height, t.width), f32) for t in tiles]
    want = M.transform(tiles, d, abcd)
    got = P.apply_all(tiles, d, abcd, ones)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    dd = DR.transform(data, (2.0, 0.5, 1.0, -0.1))
    t0 = tiles[0]
    n = t0.width * t0.height
    got = P.apply_disp(data[:n], (2.0, 0.5, 1.0, -0.1), ones[0])
    assert np.array_equal(got.view(np.uint32), dd[:n].view(np.uint32))
    # under the rule an invalid pixel becomes NaN, a valid one is transformed
    z = np.array(data[:n])
    z[:100] = 0.0
    got = P.apply_cubic(z, abcd[0], ones[0], valid=(0.0, np.inf))
    assert np.isnan(got[:100]).all() and not np.isnan(got[100:]).any()


# ---- the factor against the tile geometry -------------------------------------------------------
@pytest.mark.parametrize("cfg", ["C1", "C2"])
def test_factor_agrees_with_the_tile_geometry(cfg):
    lay = PL.config_layout(cfg)
    tiles, _ = O.make_tiles(lay)
    worst = 0.0
    for p, k in enumerate(P.layout_kf(lay)):
        g = P.geometry_norm(tiles[p])
        worst = max(worst, float(np.max(np.abs(k.astype(np.float64) - g) / g)))
        assert k.min() >= 1.0
    print(f"{cfg}: max relative |kf - |pos|| = {worst:.3e}, corner kf {k.max():.3f}")
    assert worst <= 1e-6


def test_tables_edge_cases():
    fov = (0.3, 1.5, 0.4, 1.2)
    cu, rv = P.tables(fov, 1, 7)
    assert cu.tolist() == [0.0] and rv[3] == 0.0 and rv[0] == rv[6] > 0
    cu, rv = P.tables(fov, 9, 1)
    assert rv.tolist() == [0.0] and cu[4] == 0.0
    a, b = P.tables((1.5, 0.3, 1.2, 0.4), 9, 7)  # a window given right-to-left: the same factor
    c, d = P.tables(fov, 9, 7)
    assert np.array_equal(a, c) and np.array_equal(b, d)


# ---- what the factor is worth -------------------------------------------------------------------
def _tone(z, p):
    return ((0.8 + 0.05 * (p % 3)) * z.astype(np.float64) ** (1.1 - 0.05 * (p % 2)) + 0.03
            ).astype(f32)


def _band_error(out_u16, gt, w, h):
    lv = O.level_dims(w, h, ZR, O.num_levels(w) - 1)
    got = out_u16.astype(np.float64) / 65535.0
    return float(np.mean(np.abs(got - gt)[lv.h0:lv.h1 + 1]))


def value_errors(cfg="C1"):
    """(ray tiles, planar tiles read as ray, planar tiles with the factor): mean |out - gt| over
    the band, on the default-seed scene with per-tile toned tiles."""
    lay = PL.config_layout(cfg)
    ow, ew = PL.CONFIGS[cfg]
    seeds = pf_synth.seeds_for(1)
    emap = pf_synth.baseline_emap(seeds, ew, ew // 2)[0].numpy()
    gt = pf_synth.scene_depth(seeds, ow, ow // 2)[0].numpy()
    tiles, total = O.make_tiles(lay)
    ray = O.warp_depth(gt, tiles, total)
    kfs = P.layout_kf(lay)
    toned_ray = np.empty_like(ray)
    toned_planar = np.empty_like(ray)
    for p, t in enumerate(tiles):
        s = slice(t.offset, t.offset + t.width * t.height)
        toned_ray[s] = _tone(ray[s], p)
        toned_planar[s] = _tone(ray[s] / kfs[p].reshape(-1), p)
    out_ray, _ = O.merge(emap, tiles, toned_ray.copy(), ow, ZR)
    out_asray, _ = O.merge(emap, tiles, toned_planar.copy(), ow, ZR)
    abcd = []
    for p, t in enumerate(tiles):
        xs, ys, _, _ = O.reg_samples(t, toned_planar, emap, ZR)
        c, _ = P.register(xs, ys, P.sample_K(t, emap, ZR, kfs[p]))
        abcd.append(c.astype(f32))
    fixed = P.apply_all(tiles, toned_planar, abcd, kfs)
    out_factor, _ = O.solve_depth_all(emap, tiles, fixed, ow, ZR)
    h = ow // 2
    return (_band_error(out_ray, gt, ow, h), _band_error(out_asray, gt, ow, h),
            _band_error(out_factor, gt, ow, h))


def test_value_of_the_factor_at_c1():
    e_ray, e_asray, e_factor = value_errors("C1")
    print(f"C1 mean |out - gt| over the band: ray tiles {e_ray:.5f}, planar read as ray "
          f"{e_asray:.5f}, planar with the factor {e_factor:.5f} "
          f"({e_factor / e_ray:.3f} x ray, {e_asray / e_factor:.2f} x)")
    assert e_factor <= 1.1 * e_ray
    assert e_asray >= 2.0 * e_factor
