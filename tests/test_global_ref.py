"""CPU checks of the global-registration restatement (tests/global_ref.py), which the GPU tests
(tests/test_gpu_global.py) hold csrc/pf_global.hip to bit for bit.

* Its moment-form LM from (1, 1, 1, 1) equals the oracle's pfo_lm_moments bit for bit on the C1
  tiles' sums: the new Python LM is the LM the registration path already relies on.
* On every fit case of tests/golden/global_ref.npz (tools/make_global_golden.py: the reference's
  own SolveDepthToDepth2, compiled with the vendored Ceres 1.13) the restatement's fp32 abcd
  equals the compiled reference's bit for bit and both costs agree within 1e-5 relative (the
  reference prints six digits).  Measured when the golden was recorded: 0 ulp on all four
  coefficients of all four cases (1,600 / 3,700 / 14,600 / 94,720 samples).
* Its MedianScaling and CopyInvalidPixels equal the compiled reference's maps bit for bit.
"""
import os

import numpy as np
import pytest

import global_ref as G
import pf_layouts as PL
import pf_synth
import pyoracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "global_ref.npz")
NFIT, NMAP = 4, 5


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_lm_from_ones_equals_the_oracle_on_c1_sums():
    lay = PL.config_layout("C1")
    tiles, total = O.make_tiles(lay)
    seeds = pf_synth.seeds_for(1)
    emap = pf_synth.baseline_emap(seeds, 128, 64)[0].numpy()
    gt = pf_synth.scene_depth(seeds, 512, 256)[0].numpy()
    data = O.warp_depth(gt, tiles, total, O.responses(pf_synth.responses(seeds, lay.ntiles)))
    for p, t in enumerate(tiles):
        xs, ys, _, _ = O.reg_samples(t, data, emap, PL.ZENITH_RANGE)
        assert xs.size < G.CHUNK  # one chunk: k_register's order
        S = G.moment_sums(xs, ys)
        want, ws = O.lm_moments(S)
        got, s = G.lm_moments(S, G.START_TILE)
        print(f"tile {p}: {got} {s}")
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), p
        assert s["iterations"] == ws["iterations"] and s["termination"] == ws["termination"]
        assert s["initial_cost"] == ws["initial_cost"] and s["final_cost"] == ws["final_cost"]


@pytest.mark.parametrize("k", range(NFIT))
def test_fit_equals_the_compiled_reference(golden, k):
    emap, data = golden[f"fit_emap{k}"], golden[f"fit_data{k}"]
    zr = tuple(golden["zenith_range"])
    c64, abcd, s = G.register_global(emap, data, zr)
    ref, cost = golden["fit_abcd"][k], golden["fit_cost"][k]
    ulps = G.ulp_diff(abcd, ref)
    print(f"fit {k}: restatement {abcd} reference {ref} ulp {ulps.tolist()} costs "
          f"{s['initial_cost']:.9g}->{s['final_cost']:.9g} reference {cost[0]:.6g}->{cost[1]:.6g}")
    assert np.array_equal(abcd.view(np.uint32), ref.view(np.uint32))
    assert abs(s["initial_cost"] - cost[0]) <= 1e-5 * cost[0]
    assert abs(s["final_cost"] - cost[1]) <= 1e-5 * cost[1]
    assert s["final_cost"] < s["initial_cost"]


def test_golden_covers_the_cases_it_should(golden):
    zr = tuple(golden["zenith_range"])
    shapes = [(golden[f"fit_data{k}"].shape, golden[f"fit_emap{k}"].shape) for k in range(NFIT)]
    assert shapes == [((32, 64), (8, 16)), ((50, 100), (33, 64)), ((100, 200), (25, 50, 3)),
                      ((256, 512), (64, 128))]
    xs, ys = G.samples(golden["fit_emap1"], golden["fit_data1"], zr)
    assert (xs == 1e-4).sum() > 0 and (xs == 1 - 1e-4).sum() > 0  # both clamps fire
    xs, _ = G.samples(golden["fit_emap3"], golden["fit_data3"], zr)
    assert xs.size == 94720 and xs.size % G.CHUNK != 0  # a ragged last chunk
    valid = [int(G.valid_mask(G._chan0(golden[f"map0_{k}"])).sum()) for k in range(NMAP)]
    assert valid[0] % 2 == 1 and valid[1] % 2 == 0
    ties = G._chan0(golden["map0_2"])
    assert np.unique(ties).size <= 256
    assert golden["map0_3"].shape[:2] != golden["map1_3"].shape[:2]
    assert golden["map0_4"].ndim == 3 and golden["map0_4"].shape[2] == 3


def test_ordered_sum_is_the_documented_order():
    """Chunks of 16,384; in a chunk lane l adds l, l + 256, ... from 0.0, then the halving tree;
    chunk partials in chunk order from 0.0."""
    rng = np.random.default_rng(7)
    for n in (1, 257, G.CHUNK - 1, G.CHUNK, G.CHUNK + 1, 2 * G.CHUNK + 700):
        t = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 8, n)
        total = 0.0
        for c0 in range(0, n, G.CHUNK):
            chunk = t[c0:c0 + G.CHUNK]
            part = [0.0] * 256
            for lane in range(256):
                for v in chunk[lane::256]:
                    part[lane] = part[lane] + float(v)
            stride = 128
            while stride >= 1:
                for lane in range(stride):
                    part[lane] = part[lane] + part[lane + stride]
                stride //= 2
            total = total + part[0]
        assert G.ordered_sum(t) == total


@pytest.mark.parametrize("k", range(NMAP))
def test_median_scaling_equals_the_compiled_reference(golden, k):
    m0, m1 = golden[f"map0_{k}"], golden[f"map1_{k}"]
    ok, a, b, scaled = G.median_scale(m0, m1)
    ret, ra, rb = golden["med"][k]
    assert int(ok) == int(ret)
    assert np.float32(a).view(np.uint32) == ra.view(np.uint32)
    assert np.float32(b).view(np.uint32) == rb.view(np.uint32)
    assert np.array_equal(scaled.view(np.uint32), golden[f"scaled{k}"])
    assert not np.array_equal(scaled, m0)


@pytest.mark.parametrize("k", range(NMAP))
def test_copy_invalid_equals_the_compiled_reference(golden, k):
    m0, m1 = golden[f"map0_{k}"], golden[f"map1_{k}"]
    masked = G.copy_invalid(m0, m1)
    assert np.array_equal(masked.view(np.uint32), golden[f"masked{k}"])
    assert not np.array_equal(masked, m0)


def test_rules_where_the_reference_is_undefined():
    f = np.float32
    m = np.array([[0.2, np.nan, 0.4], [0.0, 1.0, 0.3]], f)
    assert G.valid_mask(m).tolist() == [[True, False, True], [False, False, True]]
    assert G.median_of(m) == f(0.3)  # sorted valid (0.2, 0.3, 0.4), index 3 // 2
    dead = np.array([[0.0, 1.0, np.nan, 5e-5]], f)
    ok, _, _, out = G.median_scale(dead, m)
    assert not ok and np.array_equal(out.view(np.uint32), dead.view(np.uint32))
    ok, _, _, out = G.median_scale(m, dead)
    assert not ok and np.array_equal(out.view(np.uint32), m.view(np.uint32))
    # a NaN reference pixel is not copied; 0 and 1 are
    ref = np.array([[np.nan, 0.0, 1.0]], f)
    dst = np.array([[0.5, 0.5, 0.5]], f)
    assert G.copy_invalid(dst, ref).tolist() == [[0.5, 0.0, 1.0]]


def test_result_transform_rows_and_clamps():
    zr = PL.ZENITH_RANGE
    rng = np.random.default_rng(5)
    data = rng.integers(0, 65536, (50, 100)).astype(np.uint16)
    data[20, :4] = (0, 6, 65535, 65530)
    h0, h1 = G.band(50, zr)
    ident = G.result_transform(data, zr, (0, 0, 1, 0))
    assert np.array_equal(ident[:h0], data[:h0]) and np.array_equal(ident[h1 + 1:], data[h1 + 1:])
    band = data[h0:h1 + 1].astype(np.int64)
    # the identity cubic moves a value only through the X clamp and the u16 rounding
    assert np.abs(ident[h0:h1 + 1].astype(np.int64) - np.clip(band, 6, 65529)).max() <= 1
    assert (G.result_transform(data, zr, (0, 0, 0, 5))[h0:h1 + 1] == 65535).all()
    assert (G.result_transform(data, zr, (0, 0, 0, -5))[h0:h1 + 1] == 0).all()
    assert (G.result_transform(data, zr, (np.nan, 0, 0, 0))[h0:h1 + 1] == 0).all()
