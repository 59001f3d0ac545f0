"""GPU disparity-tile registration (csrc/pf_disp.hip) against its CPU restatement
(tests/disp_ref.py): coefficients, costs and iteration counts bit for bit, the fp32 transform,
and the merged panorama.

C1 shapes: 6 tiles of 256^2 (121 x 65 = 7865 samples each, inside the resident capacity with a
partly filled last row of lanes), a 128x64 baseline, 512x256 output.  The disparity tiles are the
synthetic depth tiles turned into per-tile normalised inverse depth, MiDaS' convention:
(1/max(t, 0.02) - min) / (max - min).
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import disp_ref as R  # noqa: E402
import panofuse  # noqa: E402
import pf_layouts as PL  # noqa: E402
import pf_synth  # noqa: E402
import pyoracle as O  # noqa: E402

ZR = PL.ZENITH_RANGE
DEV = "cuda:0"
OUT_W, EW = 512, 128
RESIDENT = 8192  # kDispResident of csrc/pf_disp.hip: samples kept in registers


@pytest.fixture(scope="module")
def fuser():
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected on a host without a GPU")
    return panofuse.Fuser(0)


def _to_disparity(data, tiles):
    out = np.empty_like(data)
    for t in tiles:
        n = t.width * t.height * t.channels
        inv = np.float32(1.0) / np.maximum(data[t.offset:t.offset + n], np.float32(0.02))
        lo, hi = inv.min(), inv.max()
        out[t.offset:t.offset + n] = (inv - lo) / (hi - lo)
    return out


def _inputs(lay, seed):
    tiles, total = O.make_tiles(lay)
    seeds = pf_synth.seeds_for(1, 20261015 + 1000 * seed)
    emap = pf_synth.baseline_emap(seeds, EW, EW // 2)[0].numpy()
    gt = pf_synth.scene_depth(seeds, OUT_W, OUT_W // 2)[0].numpy()
    depth = O.warp_depth(gt, tiles, total, O.responses(pf_synth.responses(seeds, lay.ntiles)))
    return tiles, emap, _to_disparity(depth, tiles)


def _reference(tiles, emap, disp):
    """Per tile: (coef64, summary row, clamped samples) of the restatement."""
    ref = []
    for t in tiles:
        xs, ys, _, _ = O.reg_samples(t, disp, emap, ZR)
        c64, s = R.fit(xs, ys)
        ref.append((c64, R.summary_row(s), xs, ys))
    return ref


@pytest.fixture(scope="module")
def c1():
    """The C1 inputs of three seeds and the restatement's fits of the first two (read-only)."""
    lay = PL.config_layout("C1")
    cases = []
    for seed in range(3):
        tiles, emap, disp = _inputs(lay, seed)
        cases.append({"tiles": tiles, "emap": emap, "disp": disp,
                      "ref": _reference(tiles, emap, disp) if seed < 2 else None})
    return lay, cases


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _register(fuser, lay, emaps, disps, apply=False):
    """register_disparity on a batch: (coeffs f32, coeffs64, summary, tiles afterwards)."""
    B = len(emaps)
    fuser.set_tiles(lay)
    t_emap = _dev(np.stack(emaps))
    t_tiles = _dev(np.stack(disps))
    cf = torch.zeros((B, lay.ntiles, 4), dtype=torch.float32, device=DEV)
    c64 = torch.zeros((B, lay.ntiles, 4), dtype=torch.float64, device=DEV)
    sm = torch.zeros((B, lay.ntiles, 4), dtype=torch.float64, device=DEV)
    fuser.register_disparity(t_emap, t_tiles, ZR, apply=apply, coeffs=cf, coeffs64=c64,
                             summary=sm)
    fuser.synchronize()
    return cf.cpu().numpy(), c64.cpu().numpy(), sm.cpu().numpy(), t_tiles.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.mark.parametrize("seed", [0, 1])
def test_coefficients_and_summary_bit_exact(fuser, c1, seed):
    lay, cases = c1
    k = cases[seed]
    cf, c64, sm, after = _register(fuser, lay, [k["emap"]], [k["disp"]])
    assert np.array_equal(after[0], k["disp"])  # apply = 0 leaves the tiles alone
    for p, (r64, rsum, _, _) in enumerate(k["ref"]):
        print(f"seed {seed} tile {p}: gpu {c64[0, p]} ref {r64} summary {sm[0, p]} ref {rsum}")
        assert np.array_equal(_bits(c64[0, p]), _bits(r64)), p
        assert np.array_equal(_bits(cf[0, p]), _bits(r64.astype(np.float32))), p
        assert np.array_equal(_bits(sm[0, p, :2]), _bits(rsum[:2])), p
        assert sm[0, p, 2] == rsum[2] and sm[0, p, 3] == rsum[3], p
        assert c64[0, p, 2] == 1.0


def test_batch_equals_single_runs(fuser, c1):
    lay, cases = c1
    emaps = [k["emap"] for k in cases]
    disps = [k["disp"] for k in cases]
    cf, c64, sm, _ = _register(fuser, lay, emaps, disps)
    for b in range(3):
        cf1, c641, sm1, _ = _register(fuser, lay, emaps[b:b + 1], disps[b:b + 1])
        assert np.array_equal(_bits(c64[b]), _bits(c641[0])), b
        assert np.array_equal(_bits(cf[b]), _bits(cf1[0])), b
        assert np.array_equal(_bits(sm[b]), _bits(sm1[0])), b
    assert not np.array_equal(c64[0], c64[1]) and not np.array_equal(c64[1], c64[2])


def test_grid_above_resident_capacity(fuser):
    """One tile whose range gives 121 x 121 samples, more than the resident capacity: the samples
    past it are gathered again in every evaluation, in the same order.  Both FOVs are 140 degrees,
    so every sample ray meets the tile plane in front."""
    full = PL.band_layout(3, 1, 256, 256, 10, 10, z_lo=30.0, z_hi=150.0)
    lay = PL.Layout("one-wide-tile", full.fovs[:1].copy(), full.ranges[:1].copy(),
                    full.tile_w[:1].copy(), full.tile_h[:1].copy())
    tiles, emap, disp = _inputs(lay, 4)
    (r64, rsum, xs, _), = _reference(tiles, emap, disp)
    assert xs.size > RESIDENT and xs.size % 256 != 0
    cf, c64, sm, _ = _register(fuser, lay, [emap], [disp])
    print(f"{xs.size} samples: gpu {c64[0, 0]} ref {r64} summary {sm[0, 0]}")
    assert np.array_equal(_bits(c64[0, 0]), _bits(r64))
    assert np.array_equal(_bits(cf[0, 0]), _bits(r64.astype(np.float32)))
    assert np.array_equal(_bits(sm[0, 0]), _bits(rsum))


STEP_TILE = 2


def _step_inputs():
    """C1's 6 tiles at 64^2 with the baseline under tile STEP_TILE's samples made a step of the
    tile's own values, y = (x > 0.5): a fit the model cannot follow, so the LM rejects steps.  The
    baseline element of each sample is read back from a baseline that holds its own element
    numbers ((i + 1) / (n + 2): exact in fp32 and inside the sample clamp)."""
    lay = PL.band_layout(3, 2, 64, 64, 10, 24, "C1:3x2@64")
    tiles, emap, disp = _inputs(lay, 5)
    n = emap.size
    probe = ((np.arange(n, dtype=np.float64) + 1.0) / (n + 2)).astype(np.float32)
    assert n + 2 < 2 ** 23 and probe[0] > 1e-4 and probe[-1] < 1 - 1e-4
    xs, ys, _, _ = O.reg_samples(tiles[STEP_TILE], disp, probe.reshape(emap.shape), ZR)
    at = np.rint(ys * (n + 2)).astype(np.int64) - 1
    assert np.array_equal(probe[at].astype(np.float64), ys)
    emap = emap.copy()
    emap.reshape(-1)[at] = (xs > 0.5).astype(np.float32)  # samples that share an element: the last
    return lay, tiles, emap, disp


def test_rejected_steps_and_iteration_cap_bit_exact(fuser):
    """A fit that runs through rejected steps to the iteration cap, which the C1 cases above do not
    reach.  The restatement's own trace has to show both before the GPU is compared with it."""
    lay, tiles, emap, disp = _step_inputs()
    ref = []
    for p, t in enumerate(tiles):
        xs, ys, _, _ = O.reg_samples(t, disp, emap, ZR)
        trace = []
        c64, s = R.fit(xs, ys, trace=trace)
        ref.append((c64, R.summary_row(s)))
        outcomes = [r["outcome"] for r in trace]
        print(f"tile {p}: {xs.size} samples, {s['termination']} after {s['iterations']}, "
              f"{outcomes.count('rejected')} rejected, {outcomes.count('invalid')} invalid")
        if p == STEP_TILE:
            assert outcomes.count("rejected") >= 1
            assert s["termination"] == "no_convergence" and s["iterations"] == R.MAX_ITER
    cf, c64, sm, _ = _register(fuser, lay, [emap], [disp])
    for p, (r64, rsum) in enumerate(ref):
        print(f"tile {p}: gpu {c64[0, p]} ref {r64} summary {sm[0, p]} ref {rsum}")
        assert np.array_equal(_bits(c64[0, p]), _bits(r64)), p
        assert np.array_equal(_bits(cf[0, p]), _bits(r64.astype(np.float32))), p
        assert np.array_equal(_bits(sm[0, p, :2]), _bits(rsum[:2])), p
        assert sm[0, p, 2] == rsum[2] and sm[0, p, 3] == rsum[3], p
        assert c64[0, p, 2] == 1.0


def _same_with_nan(got, want):
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan], want[~nan])


def test_apply_transforms_the_tiles(fuser, c1):
    lay, cases = c1
    k = cases[0]
    cf, _, _, after = _register(fuser, lay, [k["emap"]], [k["disp"]], apply=True)
    for p, t in enumerate(k["tiles"]):
        n = t.width * t.height
        want = R.transform(k["disp"][t.offset:t.offset + n], cf[0, p])
        assert _same_with_nan(after[0, t.offset:t.offset + n], want), p
    assert not np.array_equal(after[0], k["disp"])


@pytest.mark.parametrize("channels", [1, 3])
def test_disparity_transform_flat_map(fuser, channels):
    rng = np.random.default_rng(5)
    npix = 1000 * 257 + 3  # several blocks, no multiple of the block
    data = rng.uniform(-0.2, 1.2, (npix, channels)).astype(np.float32)
    f = np.float32
    data[:8, 0] = [0.0, f(1e-4), 1e-4 + 1e-6, f(1 - 1e-4), 1.0, 0.5, np.nan, -3.0]
    # (a X + b) is exactly 0 at X = 0.5: +-inf clamps to 1 / 0, and 0/0 stays NaN
    at_half = {}
    for abcd in ([3.0, 1.5, 1.0, -0.05], [2.0, -1.0, 1.0, 0.0], [2.0, -1.0, -1.0, 0.0],
                 [2.0, -1.0, 0.0, 0.25], [1.0, 1.0, 1.0, 5.0], [1.0, 1.0, 1.0, -5.0]):
        t = _dev(data)
        fuser.disparity_transform(t, abcd, channels=channels)
        fuser.synchronize()
        got = t.cpu().numpy()
        want = data.copy()
        want[:, 0] = R.transform(data[:, 0], abcd)
        assert _same_with_nan(got, want), abcd
        at_half[tuple(abcd)] = got[5, 0]
        assert np.isnan(got[6, 0])  # a NaN input stays NaN
    assert at_half[(2.0, -1.0, 1.0, 0.0)] == 1.0 and at_half[(2.0, -1.0, -1.0, 0.0)] == 0.0
    assert np.isnan(at_half[(2.0, -1.0, 0.0, 0.25)])
    assert at_half[(1.0, 1.0, 1.0, 5.0)] == 1.0 and at_half[(1.0, 1.0, 1.0, -5.0)] == 0.0


def test_merge_disparity(fuser, c1):
    lay, cases = c1
    k = cases[1]
    fuser.set_tiles(lay)
    t_emap, t_tiles = _dev(k["emap"][None]), _dev(k["disp"][None])
    out = torch.zeros((1, OUT_W // 2, OUT_W), dtype=torch.int16, device=DEV)
    cf = torch.zeros((1, lay.ntiles, 4), dtype=torch.float32, device=DEV)
    fuser.merge_disparity(t_emap, t_tiles, out, ZR, coeffs=cf)
    fuser.synchronize()
    merged = out.cpu().numpy().view(np.uint16)[0]
    assert np.array_equal(t_tiles.cpu().numpy()[0], k["disp"])  # the caller's tiles stay
    for p, (r64, _, _, _) in enumerate(k["ref"]):
        assert np.array_equal(_bits(cf.cpu().numpy()[0, p]), _bits(r64.astype(np.float32))), p

    # == register_disparity(apply = 1) followed by fuse(coeffs = None)
    work = t_tiles.clone()
    out2 = torch.zeros_like(out)
    fuser.register_disparity(t_emap, work, ZR, apply=True)
    fuser.fuse(t_emap, work, out2, ZR, coeffs=None)
    fuser.synchronize()
    assert np.array_equal(out2.cpu().numpy().view(np.uint16)[0], merged)

    # == the oracle's SolveDepthAll on tiles transformed by the restatement
    xf = k["disp"].copy()
    for p, t in enumerate(k["tiles"]):
        n = t.width * t.height
        xf[t.offset:t.offset + n] = R.transform(k["disp"][t.offset:t.offset + n],
                                                k["ref"][p][0].astype(np.float32))
    want, _ = O.solve_depth_all(k["emap"], k["tiles"], xf, OUT_W, ZR)
    assert np.array_equal(merged, want)


def test_cost_consistency(fuser, c1):
    """final <= initial, and the final cost is 0.5 sum r^2 at the returned parameters: numpy's
    own summation order differs from the kernel's by at most ~n eps relative on about 3e3
    non-negative terms (4e-13), far inside 1e-10."""
    lay, cases = c1
    k = cases[0]
    _, c64, sm, _ = _register(fuser, lay, [k["emap"]], [k["disp"]])
    for p, (_, _, xs, ys) in enumerate(k["ref"]):
        a, b, _, d = c64[0, p]
        r = 1.0 / (a * xs + b) + d - ys
        cost = 0.5 * np.sum(r * r)
        print(f"tile {p}: initial {sm[0, p, 0]} final {sm[0, p, 1]} numpy {cost}")
        assert sm[0, p, 1] <= sm[0, p, 0]
        assert abs(sm[0, p, 1] - cost) <= 1e-10 * cost, p
