"""The CPU restatement of the overlap-consistent registration (tests/consist_ref.py) on the CPU:

* with lambda = 0 it is the per-tile least squares: its coefficients agree with the oracle's
  normal-equation registration on every well-conditioned tile;
* for lambda in {0.25, 1, 4} the consistent coefficients have a pair cost no larger, and a data
  cost no smaller, than the independent ones (costs evaluated sample-wise in fp64) -- true of any
  minimiser of f + lambda g against the minimiser of f, so the margin covers rounding only;
* the fp64 projection on the fp64 grid reproduces the pair counts the feature was sized with.
"""
import functools

import numpy as np
import pytest

import consist_ref as CR
import fusion_ref as FR
import pf_layouts as PL
import pf_synth
import pyoracle as O

ZR = PL.ZENITH_RANGE
f32 = np.float32


def _tone(z, p):  # the per-tile tone curves of tests/test_planar_ref.py's value test
    return ((0.8 + 0.05 * (p % 3)) * z.astype(np.float64) ** (1.1 - 0.05 * (p % 2)) + 0.03
            ).astype(f32)


@functools.lru_cache(maxsize=None)
def toned_c1():
    """C1 with 64 x 48 tiles, toned per tile, over the (blurred) synthetic baseline: the layout,
    the oracle tiles, the data, the baseline, the fp64 pair table and every moment sum."""
    lay = PL.config_layout("C1")
    lay.tile_w[:] = 64
    lay.tile_h[:] = 48
    seeds = pf_synth.seeds_for(1)
    emap = pf_synth.baseline_emap(seeds, 128, 64)[0].numpy()
    gt = pf_synth.scene_depth(seeds, 512, 256)[0].numpy()
    tiles, total = O.make_tiles(lay)
    ray = O.warp_depth(gt, tiles, total)
    data = np.empty_like(ray)
    for p, t in enumerate(tiles):
        s = slice(t.offset, t.offset + t.width * t.height)
        data[s] = _tone(ray[s], p)
    samples = [O.reg_samples(t, data, emap, ZR)[:2] for t in tiles]
    pairs, index = CR.pair_table64(lay, ZR)
    values = CR.pair_values(CR.tile_offsets(lay), data, pairs, index)
    D = [CR.data_sums(xs, ys) for xs, ys in samples]
    Pm = [CR.pair_sums(vp, vq) for vp, vq in values]
    return {"lay": lay, "tiles": tiles, "data": data, "emap": emap, "samples": samples,
            "pairs": pairs, "values": values, "D": D, "Pm": Pm}


def test_lambda_zero_is_the_per_tile_least_squares():
    c1 = toned_c1()
    got, summary = CR.register(c1["D"], c1["Pm"], c1["pairs"], 0.0)
    assert summary[3] == 0.0
    skipped = 0
    for p, t in enumerate(c1["tiles"]):
        k = FR.kappa(c1["samples"][p][0])
        if not k < FR.KAPPA_MAX:
            skipped += 1
            continue
        want, _, deg = O.register_tile(t, c1["data"], c1["emap"], ZR, 3, "normal")
        assert deg == 3
        rel = FR.rel_diff(got[p], want).max()
        print(f"tile {p}: kappa {k:.3g}, rel {rel:.3g}")
        assert rel <= FR.ABCD_RTOL, (p, got[p], want)
    assert 2 * skipped < len(c1["tiles"]), skipped


def _sample_costs(c1, c):
    """(data cost, pair cost) of coefficients c [nt][4], sample by sample in fp64."""
    def row(X):
        return np.stack([X * X * X, X * X, X, np.ones_like(X)], 1)
    dc = sum(float((((row(xs) @ c[p]) - ys) ** 2).sum())
             for p, (xs, ys) in enumerate(c1["samples"]))
    pc = 0.0
    for (p, q, _, _), (vp, vq) in zip(c1["pairs"].tolist(), c1["values"]):
        pc += float(((row(CR.clamp(vp)) @ c[p] - row(CR.clamp(vq)) @ c[q]) ** 2).sum())
    return dc, pc


@pytest.mark.parametrize("lam", [0.25, 1.0, 4.0])
def test_consistency_trades_data_cost_for_pair_cost(lam):
    c1 = toned_c1()
    ind, _ = CR.register(c1["D"], c1["Pm"], c1["pairs"], 0.0)
    con, summary = CR.register(c1["D"], c1["Pm"], c1["pairs"], lam)
    assert summary[3] == 0.0
    d0, p0 = _sample_costs(c1, ind)
    d1, p1 = _sample_costs(c1, con)
    print(f"lambda {lam}: data cost {d0:.6g} -> {d1:.6g}, pair cost {p0:.6g} -> {p1:.6g}; "
          f"summary {summary}")
    assert p1 <= p0 * (1 + 1e-9)
    assert d1 >= d0 * (1 - 1e-9)
    # the summary's moment-form costs are the same numbers up to the sums' rounding
    assert abs(summary[0] - d1) <= 1e-6 * d1 and abs(summary[1] - p1) <= 1e-6 * max(p1, d1)
    assert summary[2] == sum(len(v[0]) for v in c1["values"])


def test_singular_blocks_give_none():
    c1 = toned_c1()
    D = [d.copy() for d in c1["D"]]
    xs = np.full(100, 0.5)
    D[2] = CR.data_sums(xs, xs)  # a constant tile: its 4 x 4 block has rank 1
    Pm = [np.zeros(36) for _ in c1["Pm"]]
    c, summary = CR.register(D, Pm, c1["pairs"], 1.0)
    assert np.isnan(c).all() and summary[3] == 1.0 and np.isnan(summary[:2]).all()


def _layout(name):
    if name == "C1":
        return PL.band_layout(3, 2, 64, 48, 10, 24)
    if name == "LERES":
        return PL.leres_layout(64, 48)
    return PL.band_layout(5, 4, 64, 48, 3, 12)


# layout -> tiles, registration samples, ordered pairs, pair samples, smallest / largest pair
COUNTS = {
    "C1": (6, 47190, 30, 33490, 46, 2480),
    "LERES": (15, 47815, 90, 47783, 7, 2443),
    "C2": (20, 48545, 130, 50884, 15, 1021),
}


@pytest.mark.parametrize("name", sorted(COUNTS))
def test_pair_counts(name):
    lay = _layout(name)
    pairs, index = CR.pair_table64(lay, ZR, grid=CR.reg_grid64)
    nreg = sum(CR.reg_grid64(r, ZR)[0].size for r in lay.capped_ranges())
    got = (lay.ntiles, nreg, len(pairs), len(index), int(pairs[:, 3].min()),
           int(pairs[:, 3].max()))
    assert got == COUNTS[name]
    partners = [set(pairs[pairs[:, 0] == p, 1]) | set(pairs[pairs[:, 1] == p, 0])
                for p in range(lay.ntiles)]
    assert min(len(s) for s in partners) >= 5
    # the table is sorted, and first / count tile it
    keys = [(int(a), int(b)) for a, b in pairs[:, :2]]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    assert np.array_equal(pairs[:, 2], np.concatenate([[0], np.cumsum(pairs[:, 3])[:-1]]))
