"""GPU robust tile registration (pf_set_register_loss: csrc/pf_robust.hip and the loss
instantiation of csrc/pf_disp.hip) against its CPU restatement (tests/robust_ref.py):
coefficients and the 6-entry summary bit for bit, the merged panorama, the validity rule, the
refusals, and the default path left as it was.

Shapes: C1 with 6 tiles of 64^2 (121 x 65 = 7865 samples each, inside the resident capacity with
a partly filled last row of lanes), a 40 x 20 baseline, 256 x 128 output; and one tile with
121 x 121 = 14641 samples, above the resident capacity of 8192 and no multiple of 256.

Planted outliers.  The bit comparisons replace 10 % of every tile's pixels by U(0, 1) (outliers in
x).  The fused-panorama comparison replaces 10 % of the baseline's pixels instead: outliers in the
y values, the experiment the loss was asked for.  A loss protects the fit, not the fusion's own
reads: an outlier pixel of a tile also enters the Laplacian targets directly, whatever the
coefficients, and with those the CPU composition's band error moves either way (seeds 0-2 at
a = 0.02: 0.0270 / 0.0303, 0.0244 / 0.0242, 0.0162 / 0.0176 with Huber / without), while with the
baseline's it is lower with Huber on every seed (0.0203 / 0.0295, 0.0233 / 0.0299,
0.0249 / 0.0262).
"""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import fusion_ref as FR  # noqa: E402
import panofuse  # noqa: E402
import pf_layouts as PL  # noqa: E402
import pf_synth  # noqa: E402
import pyoracle as O  # noqa: E402
import robust_ref as R  # noqa: E402

ZR = PL.ZENITH_RANGE
DEV = "cuda:0"
W, H, EW, EH = 256, 128, 40, 20
RESIDENT = 8192  # kDispResident of csrc/pf_lm.hpp
A = 0.02
LOSSES = [("huber", A), ("softl1", A)]
INF = float("inf")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "c1_merge.npz")


@pytest.fixture(scope="module")
def fuser():
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected on a host without a GPU")
    fz = panofuse.Fuser(0)
    yield fz
    fz.close()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _to_disparity(data, tiles):
    """Per-tile normalised inverse depth, MiDaS' convention (as tests/test_gpu_disp.py)."""
    out = np.empty_like(data)
    for t in tiles:
        n = t.width * t.height * t.channels
        inv = np.float32(1.0) / np.maximum(data[t.offset:t.offset + n], np.float32(0.02))
        lo, hi = inv.min(), inv.max()
        out[t.offset:t.offset + n] = (inv - lo) / (hi - lo)
    return out


def _inputs(lay, seed, ew, eh, ow, oh):
    """Synthetic (oracle tiles, emap, gt, clean depth tiles, depth tiles with planted outliers,
    disparity tiles with planted outliers, emap with planted outliers)."""
    tiles, total = O.make_tiles(lay)
    seeds = pf_synth.seeds_for(1, 20261020 + 1000 * seed)
    emap = pf_synth.baseline_emap(seeds, ew, eh)[0].numpy()
    gt = pf_synth.scene_depth(seeds, ow, oh)[0].numpy()
    clean = O.warp_depth(gt, tiles, total, O.responses(pf_synth.responses(seeds, lay.ntiles)))
    disp = _to_disparity(clean, tiles)
    rng = np.random.default_rng(500 + seed)
    hit = rng.random(emap.shape) < 0.10
    emap_out = emap.copy()
    emap_out[hit] = rng.uniform(0, 1, int(hit.sum())).astype(np.float32)
    return (tiles, emap, gt, clean, R.plant_tile_outliers(clean, tiles, 77 + seed),
            R.plant_tile_outliers(disp, tiles, 177 + seed), emap_out)


@pytest.fixture(scope="module")
def c1():
    """The C1 inputs of three seeds (read-only)."""
    lay = FR.layout("C1", (64, 64))
    return lay, [_inputs(lay, seed, EW, EH, W, H) for seed in range(3)]


@pytest.fixture(scope="module")
def refs():
    """Restatement fits, computed once per (model, seed, loss) and shared."""
    cache = {}

    def get(key, tiles, emap, data, kind, a, model):
        if key not in cache:
            fits = []
            for t in tiles:
                xs, ys, _, _ = O.reg_samples(t, data, emap, ZR)
                fits.append(R.fit(xs, ys, kind, a, model))
            cache[key] = fits
        return cache[key]
    return get


def _register(fuser, lay, emaps, datas, model, apply=False):
    """register / register_disparity on a batch: (coeffs f32, coeffs64, summary [B, n, 6])."""
    B = len(emaps)
    fuser.set_tiles(lay)
    t_emap, t_tiles = _dev(np.stack(emaps)), _dev(np.stack(datas))
    cf = torch.zeros((B, lay.ntiles, 4), dtype=torch.float32, device=DEV)
    c64 = torch.zeros((B, lay.ntiles, 4), dtype=torch.float64, device=DEV)
    sm = torch.full((B, lay.ntiles, 6), -1.0, dtype=torch.float64, device=DEV)
    call = fuser.register if model == "cubic" else fuser.register_disparity
    call(t_emap, t_tiles, ZR, apply=apply, coeffs=cf, coeffs64=c64, summary=sm)
    fuser.synchronize()
    return cf.cpu().numpy(), c64.cpu().numpy(), sm.cpu().numpy()


def _same(got, want):
    """Bit equality, any NaN equal to any NaN."""
    nan = np.isnan(want)
    return (np.array_equal(np.isnan(got), nan)
            and np.array_equal(_bits(got[~nan]), _bits(want[~nan])))


def _check_tile(tag, cf, c64, sm, fit):
    r64, s = fit
    row = R.summary_row(s)
    print(f"{tag}: gpu {c64} ref {r64}\n   summary gpu {sm} ref {row}")
    assert _same(c64, r64), tag
    assert _same(cf, r64.astype(np.float32)), tag
    assert _same(sm, row), tag


@pytest.mark.parametrize("model", ["cubic", "disparity"])
@pytest.mark.parametrize("kind,a", LOSSES)
def test_coefficients_and_summary_bit_exact(fuser, c1, refs, kind, a, model):
    lay, cases = c1
    tiles, emap, _, _, depth, disp, _ = cases[0]
    data = depth if model == "cubic" else disp
    fuser.set_register_loss(kind, a)
    try:
        cf, c64, sm = _register(fuser, lay, [emap], [data], model)
    finally:
        fuser.set_register_loss(None)
    fits = refs((model, 0, kind), tiles, emap, data, kind, a, model)
    for p in range(lay.ntiles):
        _check_tile(f"{model} {kind} tile {p}", cf[0, p], c64[0, p], sm[0, p], fits[p])
        ns = fits[p][1]["used"]
        assert ns == 7865 and sm[0, p, 4] == ns and 0 < sm[0, p, 5] < ns  # the loss is active
    if model == "disparity":
        assert np.all(c64[0, :, 2] == 1.0)


@pytest.mark.parametrize("model", ["cubic", "disparity"])
def test_batch_equals_single_runs(fuser, c1, refs, model):
    lay, cases = c1
    emaps = [k[1] for k in cases]
    datas = [k[4] if model == "cubic" else k[5] for k in cases]
    fuser.set_register_loss("huber", A)
    try:
        cf, c64, sm = _register(fuser, lay, emaps, datas, model)
        singles = [_register(fuser, lay, emaps[b:b + 1], datas[b:b + 1], model) for b in range(3)]
    finally:
        fuser.set_register_loss(None)
    for b in range(3):
        assert _same(c64[b], singles[b][1][0]) and _same(cf[b], singles[b][0][0]), b
        assert _same(sm[b], singles[b][2][0]), b
    assert not np.array_equal(c64[0], c64[1]) and not np.array_equal(c64[1], c64[2])
    # panorama 2 of the batch against the restatement
    fits = refs((model, 2, "huber"), cases[2][0], emaps[2], datas[2], "huber", A, model)
    for p in range(lay.ntiles):
        _check_tile(f"{model} batch tile {p}", cf[2, p], c64[2, p], sm[2, p], fits[p])


@pytest.mark.parametrize("model", ["cubic", "disparity"])
@pytest.mark.parametrize("kind,a", LOSSES)
def test_grid_above_resident_capacity(fuser, kind, a, model):
    """One tile whose range gives 121 x 121 samples, more than the resident capacity: the samples
    past it are gathered again in every evaluation, in the same order."""
    full = PL.band_layout(3, 1, 256, 256, 10, 10, z_lo=30.0, z_hi=150.0)
    lay = PL.Layout("one-wide-tile", full.fovs[:1].copy(), full.ranges[:1].copy(),
                    full.tile_w[:1].copy(), full.tile_h[:1].copy())
    tiles, emap, _, _, depth, disp, _ = _inputs(lay, 4, 128, 64, 512, 256)
    data = depth if model == "cubic" else disp
    xs, ys, _, _ = O.reg_samples(tiles[0], data, emap, ZR)
    assert xs.size > RESIDENT and xs.size % 256 != 0
    fit = R.fit(xs, ys, kind, a, model)
    fuser.set_register_loss(kind, a)
    try:
        cf, c64, sm = _register(fuser, lay, [emap], [data], model)
    finally:
        fuser.set_register_loss(None)
    _check_tile(f"{model} {kind} {xs.size} samples", cf[0, 0], c64[0, 0], sm[0, 0], fit)
    assert sm[0, 0, 4] == xs.size and 0 < sm[0, 0, 5] < xs.size


def _band_error(out_u16, gt):
    lv = O.level_dims(W, H, ZR, O.num_levels(W) - 1)
    got = out_u16.astype(np.float64) / 65535.0
    return float(np.mean(np.abs(got - gt)[lv.h0:lv.h1 + 1]))


def _merge(fuser, emap, data):
    out = torch.zeros((1, H, W), dtype=torch.int16, device=DEV)
    cf = torch.zeros((1, 6, 4), dtype=torch.float32, device=DEV)
    t_tiles = _dev(data[None])
    fuser.merge(_dev(emap[None]), t_tiles, out, ZR, coeffs=cf)
    fuser.synchronize()
    assert np.array_equal(t_tiles.cpu().numpy()[0], data)  # the caller's tiles stay
    return out.cpu().numpy().view(np.uint16)[0], cf.cpu().numpy()[0]


def test_merge_with_huber(fuser, c1, refs):
    """pf_merge under Huber == the restatement's coefficients fed to the oracle's transform and
    fusion, bit for bit; and with the planted outliers the fused panorama is closer to the ground
    truth with Huber than without, on the GPU and in the CPU composition alike."""
    lay, cases = c1
    tiles, _, gt, depth, _, _, emap = cases[1]  # clean tiles, outliers in the baseline
    fuser.set_tiles(lay)
    fuser.set_register_loss("huber", A)
    try:
        robust, cf = _merge(fuser, emap, depth)
    finally:
        fuser.set_register_loss(None)
    plain, cf_plain = _merge(fuser, emap, depth)

    fits = refs(("cubic-emap", 1, "huber"), tiles, emap, depth, "huber", A, "cubic")
    abcd = np.stack([f[0].astype(np.float32) for f in fits])
    assert np.array_equal(_bits(cf), _bits(abcd))
    xf = depth.copy()
    for p in range(lay.ntiles):
        O.depth_to_depth(tiles[p], xf, abcd[p])
    want, _ = O.solve_depth_all(emap, tiles, xf, W, ZR)
    assert np.array_equal(robust, want)
    want_plain, abcd_plain = O.merge(emap, tiles, depth.copy(), W, ZR)
    assert np.array_equal(plain, want_plain) and np.array_equal(cf_plain, abcd_plain)

    e_robust, e_plain = _band_error(robust, gt), _band_error(plain, gt)
    c_robust, c_plain = _band_error(want, gt), _band_error(want_plain, gt)
    print(f"mean |out - gt| over the band: gpu huber {e_robust:.6f} none {e_plain:.6f}; "
          f"cpu huber {c_robust:.6f} none {c_plain:.6f}")
    assert e_robust < e_plain and c_robust < c_plain


def test_validity_rule(fuser, c1):
    """PF_VALID_RANGE(0, inf) with a zeroed rectangle in tile 0 and tile 4 zeroed but for three
    pixels' worth of samples: skipped samples are left out of summary[4], the fit is the
    restatement's on the kept samples, too few samples give NaN and termination 5."""
    lay, cases = c1
    tiles, emap, _, _, depth, _, _ = cases[0]
    d = depth.copy().reshape(6, 64, 64)
    d[0, 10:40, 20:64] = 0.0
    d[4] = 0.0
    data = d.reshape(-1)
    nan = np.where(data > 0, data, np.float32(np.nan))  # what the rule rejects, as NaN
    fuser.set_tile_validity(0.0, INF)
    fuser.set_register_loss("huber", A)
    try:
        cf, c64, sm = _register(fuser, lay, [emap], [data], "cubic")
    finally:
        fuser.set_register_loss(None)
        fuser.set_tile_validity(None, None)
    for p in range(lay.ntiles):
        xs, ys, _, _ = O.reg_samples(tiles[p], nan, emap, ZR)
        valid = ~np.isnan(xs) & np.isfinite(ys)
        fit = R.fit(xs, ys, "huber", A, "cubic", valid=valid)
        _check_tile(f"masked tile {p}", cf[0, p], c64[0, p], sm[0, p], fit)
        assert sm[0, p, 4] == np.count_nonzero(valid)
    assert 4 <= sm[0, 0, 4] < 7865 and sm[0, 1, 4] > 7000
    assert sm[0, 4, 4] == 0 and sm[0, 4, 3] == 5 and np.isnan(c64[0, 4]).all()
    assert np.isnan(cf[0, 4]).all()


def test_loss_none_after_a_loss_is_the_default_path(fuser):
    """PF_LOSS_NONE after a loss was set: the golden bits and the per-stage launch counts of a
    context that never set one."""
    g = np.load(GOLDEN)
    emap = (g["emap_u16"].astype(np.float32) / np.float32(65535.0)).astype(np.float32)
    data = (g["tiles_u8"].astype(np.float32) / np.float32(255.0)).astype(np.float32)
    lay = PL.config_layout("C1")

    def run(fz):
        out = torch.zeros((1, 256, 512), dtype=torch.int16, device=DEV)
        cf = torch.zeros((1, 6, 4), dtype=torch.float32, device=DEV)
        fz.profile(True)
        fz.merge(_dev(emap[None]), _dev(data.reshape(1, -1)), out, ZR, coeffs=cf)
        fz.synchronize()
        prof = fz.profile_read()
        fz.profile(False)
        return out.cpu().numpy().view(np.uint16)[0], cf.cpu().numpy()[0], prof

    fuser.set_tiles(lay)
    fuser.set_register_loss("huber", A)
    on = run(fuser)
    fuser.set_register_loss(None)
    got = run(fuser)
    fresh = panofuse.Fuser(0)
    fresh.set_tiles(lay)
    ref = run(fresh)
    fresh.close()
    assert np.array_equal(got[0], g["out_u16"]) and np.array_equal(got[1], g["abcd"])
    assert np.array_equal(ref[0], g["out_u16"])
    assert {k: v[2] for k, v in got[2].items()} == {k: v[2] for k, v in ref[2].items()}
    # with the loss on, the register stage is still one launch, and the result another one
    assert on[2]["register"][2] == ref[2]["register"][2]
    assert not np.array_equal(on[1], g["abcd"])


def test_refusals(fuser, c1):
    lay, cases = c1
    _, emap, _, _, depth, _, _ = cases[0]
    fuser.set_tiles(lay)
    e, t = _dev(emap[None]), _dev(depth[None])
    sm = torch.zeros((1, 6, 6), dtype=torch.float64, device=DEV)
    out = torch.zeros((1, H, W), dtype=torch.int16, device=DEV)

    def refused(code, call, names="pf_set_register_loss"):
        with pytest.raises(panofuse.PanofuseError) as err:
            call()
        assert err.value.code == code, str(err.value)
        assert names in str(err.value), str(err.value)

    # summary without a loss
    refused(panofuse.PF_EINVAL, lambda: fuser.register(e, t, ZR, apply=False, summary=sm))
    # a <= 0, NaN, inf, an unknown kind
    for bad in (0.0, -1.0, float("nan"), INF):
        refused(panofuse.PF_EINVAL, lambda: fuser.set_register_loss("huber", bad))
    with pytest.raises(panofuse.PanofuseError) as err:
        fuser._check(fuser.L.pf_set_register_loss(fuser.h, 7, 1.0))
    assert err.value.code == panofuse.PF_EINVAL
    fuser.set_register_loss("huber", A)
    try:
        refused(panofuse.PF_ESTATE, lambda: fuser.register_joint(e, t, ZR, [0, 1]))
        refused(panofuse.PF_ESTATE, lambda: fuser.register_global(e, out, ZR))
        refused(panofuse.PF_EINVAL, lambda: fuser.register(e, t, ZR, degree=1, apply=False))
        fuser.set_solver("normal")
        refused(panofuse.PF_EINVAL, lambda: fuser.register(e, t, ZR, apply=False))
        refused(panofuse.PF_EINVAL, lambda: fuser.merge(e, t, out, ZR))
        fuser.set_solver("lm")
    finally:
        fuser.set_solver("lm")
        fuser.set_register_loss(None)
    # unset: they run again
    fuser.register_joint(e, t, ZR, [0, 1])
    fuser.register(e, t, ZR, degree=1, apply=False)
    fuser.synchronize()
