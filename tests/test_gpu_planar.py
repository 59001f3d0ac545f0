"""Planar-depth tiles on the GPU (pf_set_tile_depth) against their CPU restatement
(tests/planar_ref.py), bit for bit: the tables and the factor, the moment-form registration (both
solvers, degree 1, batches, the validity rule), the sample-wise cubic under Huber / SoftLOne and
the disparity fit, apply, merge, the refusals, and the default path left as it was.

Shapes: C1 (6 tiles of 256^2 whose ranges give 121 x 65 = 7865 samples, inside the resident
capacity of 8192 with a partly filled last row of lanes; 512 x 256 output, 128 x 64 baseline), two
64^2 tiles with 20 x 20 degree ranges (441 samples: fewer than two rows of lanes), and one tile with
121 x 121 = 14641 samples, above the capacity and no multiple of 256.
"""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import mask_ref as M  # noqa: E402
import panofuse  # noqa: E402
import pf_layouts as PL  # noqa: E402
import pf_synth  # noqa: E402
import planar_ref as P  # noqa: E402
import pyoracle as O  # noqa: E402
import robust_ref as RR  # noqa: E402

ZR = PL.ZENITH_RANGE
DEV = "cuda:0"
W, H, EW, EH = 512, 256, 128, 64
RESIDENT = 8192  # kDispResident of csrc/pf_lm.hpp: the planar kernels keep it (K is loaded per pass)
A = 0.02
INF = float("inf")
f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "c1_merge.npz")


@pytest.fixture(scope="module")
def fuser():
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected on a host without a GPU")
    fz = panofuse.Fuser(0)
    fz.set_tile_depth("planar")
    yield fz
    fz.close()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same(got, want):
    """Bit equality, any NaN equal to any NaN."""
    nan = np.isnan(want)
    return (np.array_equal(np.isnan(got), nan)
            and np.array_equal(_bits(got[~nan]), _bits(want[~nan])))


def _to_disparity(data, tiles):
    out = np.empty_like(data)
    for t in tiles:
        n = t.width * t.height * t.channels
        inv = f32(1.0) / np.maximum(data[t.offset:t.offset + n], f32(0.02))
        lo, hi = inv.min(), inv.max()
        out[t.offset:t.offset + n] = (inv - lo) / (hi - lo)
    return out


class Case:
    """A layout with its oracle tiles, factor, per-sample K and the inputs of `nb` panoramas:
    planar-depth tiles (the warped ray distance over kf, toned per tile) and their disparity."""

    def __init__(self, lay, ew, eh, ow, oh, nb=1, seed0=0):
        self.lay = lay
        self.tiles, total = O.make_tiles(lay)
        self.kf = P.layout_kf(lay)
        self.emaps, self.depth, self.disp = [], [], []
        for b in range(nb):
            seeds = pf_synth.seeds_for(1, 20261020 + 1000 * (seed0 + b))
            emap = pf_synth.baseline_emap(seeds, ew, eh)[0].numpy()
            gt = pf_synth.scene_depth(seeds, ow, oh)[0].numpy()
            ray = O.warp_depth(gt, self.tiles, total,
                               O.responses(pf_synth.responses(seeds, lay.ntiles)))
            d = np.empty_like(ray)
            for p, t in enumerate(self.tiles):
                s = slice(t.offset, t.offset + t.width * t.height)
                d[s] = ray[s] / self.kf[p].reshape(-1)
            self.emaps.append(emap)
            self.depth.append(d)
            self.disp.append(_to_disparity(d, self.tiles))
        self.K = [P.sample_K(t, self.emaps[0], ZR, self.kf[p]) for p, t in enumerate(self.tiles)]
        self._samples = {}

    def samples(self, b, p, data=None, key="depth"):
        """(xs, ys) of tile p of panorama b, cached per key."""
        k = (b, p, key)
        if k not in self._samples:
            d = self.depth[b] if data is None else data
            xs, ys, _, _ = O.reg_samples(self.tiles[p], d, self.emaps[b], ZR)
            self._samples[k] = (xs, ys)
        return self._samples[k]


@pytest.fixture(scope="module")
def c1():
    return Case(PL.config_layout("C1"), EW, EH, W, H, nb=3)


@pytest.fixture(scope="module")
def small():
    """Two 64^2 tiles with 20 x 20 degree ranges: 21 x 21 = 441 samples each."""
    full = PL.band_layout(18, 6, 64, 64, 5, 5, z_lo=30.0, z_hi=150.0)
    lay = PL.Layout("two-small-tiles", full.fovs[18:20].copy(), full.ranges[18:20].copy(),
                    full.tile_w[:2].copy(), full.tile_h[:2].copy())
    c = Case(lay, EW, EH, W, H, seed0=5)
    assert c.K[0].size == 441
    return c


@pytest.fixture(scope="module")
def wide():
    """One 256^2 tile with 121 x 121 = 14641 samples: above the resident capacity."""
    full = PL.band_layout(3, 1, 256, 256, 10, 10, z_lo=30.0, z_hi=150.0)
    lay = PL.Layout("one-wide-tile", full.fovs[:1].copy(), full.ranges[:1].copy(),
                    full.tile_w[:1].copy(), full.tile_h[:1].copy())
    c = Case(lay, EW, EH, W, H, seed0=4)
    assert c.K[0].size > RESIDENT and c.K[0].size % 256 != 0
    return c


def _register(fuser, case, datas, model="cubic", summary=0, apply=False, **kw):
    """register / register_disparity on the case's panoramas: (coeffs f32, coeffs64, summary or
    None, tiles after the call)."""
    B = len(datas)
    n = case.lay.ntiles
    fuser.set_tiles(case.lay)
    t_emap, t_tiles = _dev(np.stack(case.emaps[:B])), _dev(np.stack(datas))
    cf = torch.zeros((B, n, 4), dtype=torch.float32, device=DEV)
    c64 = torch.zeros((B, n, 4), dtype=torch.float64, device=DEV)
    sm = torch.full((B, n, summary), -1.0, dtype=torch.float64, device=DEV) if summary else None
    call = fuser.register if model == "cubic" else fuser.register_disparity
    call(t_emap, t_tiles, ZR, apply=apply, coeffs=cf, coeffs64=c64, summary=sm, **kw)
    fuser.synchronize()
    return (cf.cpu().numpy(), c64.cpu().numpy(), sm.cpu().numpy() if summary else None,
            t_tiles.cpu().numpy())


# ---- 1. tables and factor -----------------------------------------------------------------------
def _ulps(a, b):
    return int(np.max(np.abs(a.view(np.int64) - b.view(np.int64))))


def test_tables_and_factor(fuser, c1):
    lay = c1.lay
    fuser.set_tiles(lay)
    got = fuser.tile_ray_factor().cpu().numpy()
    off = 0
    for p in range(lay.ntiles):
        w, h = int(lay.tile_w[p]), int(lay.tile_h[p])
        cu, rv = fuser.tile_ray_tables(p)
        wcu, wrv = P.tables(lay.fovs[p], w, h)
        assert cu.shape == (w,) and rv.shape == (h,)
        assert _ulps(cu, wcu) <= 4 and _ulps(rv, wrv) <= 4, (p, _ulps(cu, wcu), _ulps(rv, wrv))
        want = P.kf(cu, rv)  # from the library's own tables: bit for bit
        assert np.array_equal(_bits(got[off:off + w * h]), _bits(want.reshape(-1))), p
        off += w * h
    assert off == got.size and got.min() >= 1.0 and got.max() > 3.0
    # the factor works in ray mode too
    fuser.set_tile_depth("ray")
    try:
        assert np.array_equal(fuser.tile_ray_factor().cpu().numpy(), got)
    finally:
        fuser.set_tile_depth("planar")
    with pytest.raises(panofuse.PanofuseError) as err:
        fuser._check(fuser.L.pf_set_tile_depth(fuser.h, 2))
    assert err.value.code == panofuse.PF_EINVAL
    with pytest.raises(ValueError):
        fuser.set_tile_depth("plane")


# ---- 2. the moment-form registration ------------------------------------------------------------
@pytest.mark.parametrize("degree,solver", [(3, "lm"), (3, "normal"), (1, "lm")])
def test_register_batch_bit_exact(fuser, c1, degree, solver):
    fuser.set_solver(solver)
    try:
        cf, c64, _, after = _register(fuser, c1, c1.depth, degree=degree)
    finally:
        fuser.set_solver("lm")
    assert np.array_equal(after, np.stack(c1.depth))  # apply=False leaves the tiles
    for b in range(3):
        for p in range(c1.lay.ntiles):
            xs, ys = c1.samples(b, p)
            want, _ = P.register(xs, ys, c1.K[p], None, degree, solver)
            assert _same(c64[b, p], want), (b, p, c64[b, p], want)
            assert _same(cf[b, p], want.astype(f32)), (b, p)
    assert not np.array_equal(c64[0], c64[1]) and not np.array_equal(c64[1], c64[2])
    if degree == 1:
        assert np.all(c64[:, :, :2] == 0.0)
    # the factor matters: the ray-mode fit of the same tiles is another one
    fuser.set_tile_depth("ray")
    try:
        _, r64, _, _ = _register(fuser, c1, c1.depth[:1], degree=degree)
    finally:
        fuser.set_tile_depth("planar")
    assert not np.array_equal(r64[0], c64[0])


def _holed(case, b=0):
    """Panorama b's tiles with mask_ref's `rect` hole and a whole tile as NaN."""
    d = M.with_holes(case.depth[b], "rect")
    return M.with_holes(d, "tile")


@pytest.mark.parametrize("degree,solver", [(3, "lm"), (1, "normal")])
def test_register_under_the_validity_rule(fuser, c1, degree, solver):
    data = _holed(c1)
    fuser.set_tile_validity(-INF, INF)
    fuser.set_solver(solver)
    try:
        cf, c64, _, _ = _register(fuser, c1, [data], degree=degree)
    finally:
        fuser.set_solver("lm")
        fuser.set_tile_validity(None, None)
    for p in range(c1.lay.ntiles):
        xs, ys = c1.samples(0, p, data, "holed")
        valid = ~np.isnan(xs) & np.isfinite(ys)
        want, S = P.register(xs, ys, c1.K[p], valid, degree, solver)
        assert S[15] == np.count_nonzero(valid)
        assert _same(c64[0, p], want) and _same(cf[0, p], want.astype(f32)), (p, c64[0, p], want)
    assert np.isnan(c64[0, M.ALL_TILE]).all() and np.isnan(cf[0, M.ALL_TILE]).all()
    assert np.isfinite(c64[0, 0]).all()


# ---- 3. Huber and SoftLOne ----------------------------------------------------------------------
def _check_fit(tag, cf, c64, sm, fit, row):
    r64, s = fit
    want = row(s)
    print(f"{tag}: gpu {c64} ref {r64}\n   summary gpu {sm} ref {want}")
    assert _same(c64, r64), tag
    assert _same(cf, r64.astype(f32)), tag
    if sm is not None:
        assert _same(sm, want), tag


@pytest.mark.parametrize("kind", ["huber", "softl1"])
@pytest.mark.parametrize("which", ["c1", "small", "wide"])
def test_robust_cubic_bit_exact(fuser, request, which, kind):
    case = request.getfixturevalue(which)
    data = RR.plant_tile_outliers(case.depth[0], case.tiles, 77)
    fuser.set_register_loss(kind, A)
    try:
        cf, c64, sm, _ = _register(fuser, case, [data], summary=6)
    finally:
        fuser.set_register_loss(None)
    for p in range(case.lay.ntiles):
        xs, ys = case.samples(0, p, data, "outliers")
        fit = P.fit(xs, ys, case.K[p], kind, A, "cubic")
        _check_fit(f"{which} {kind} tile {p}", cf[0, p], c64[0, p], sm[0, p], fit, RR.summary_row)
        assert sm[0, p, 4] == xs.size and 0 < sm[0, p, 5] < xs.size  # the loss is active


def test_robust_cubic_under_the_validity_rule(fuser, c1):
    data = _holed(c1)
    fuser.set_tile_validity(-INF, INF)
    fuser.set_register_loss("huber", A)
    try:
        cf, c64, sm, _ = _register(fuser, c1, [data], summary=6)
    finally:
        fuser.set_register_loss(None)
        fuser.set_tile_validity(None, None)
    for p in range(c1.lay.ntiles):
        xs, ys = c1.samples(0, p, data, "holed")
        valid = ~np.isnan(xs) & np.isfinite(ys)
        fit = P.fit(xs, ys, c1.K[p], "huber", A, "cubic", valid=valid)
        _check_fit(f"masked tile {p}", cf[0, p], c64[0, p], sm[0, p], fit, RR.summary_row)
    assert sm[0, M.ALL_TILE, 4] == 0 and sm[0, M.ALL_TILE, 3] == 5
    assert np.isnan(c64[0, M.ALL_TILE]).all()


# ---- 4. the disparity model ---------------------------------------------------------------------
@pytest.mark.parametrize("kind", [None, "huber"])
@pytest.mark.parametrize("which", ["c1", "wide"])
def test_register_disparity_bit_exact(fuser, request, which, kind):
    import disp_ref as DR
    case = request.getfixturevalue(which)
    data = case.disp[0]
    width = 6 if kind else 4
    fuser.set_register_loss(kind, A)
    try:
        cf, c64, sm, _ = _register(fuser, case, [data], "disparity", summary=width)
    finally:
        fuser.set_register_loss(None)
    row = RR.summary_row if kind else DR.summary_row
    for p in range(case.lay.ntiles):
        xs, ys = case.samples(0, p, data, "disp")
        fit = P.fit(xs, ys, case.K[p], kind, A, "disparity")
        _check_fit(f"{which} disparity {kind} tile {p}", cf[0, p], c64[0, p], sm[0, p], fit, row)
    assert np.all(c64[0, :, 2] == 1.0)
    fuser.set_tile_validity(0.0, INF)  # still refused under the rule, as in ray mode
    try:
        with pytest.raises(panofuse.PanofuseError) as err:
            _register(fuser, case, [data], "disparity")
        assert err.value.code == panofuse.PF_ESTATE
    finally:
        fuser.set_tile_validity(None, None)


# ---- 5. apply -----------------------------------------------------------------------------------
def _unsampled_pixels(case, p, count=5):
    """Pixels of tile p that no registration sample reads."""
    t = case.tiles[p]
    used = np.zeros(t.width * t.height, bool)
    used[P.sample_pixels(t, case.emaps[0], ZR)] = True
    return np.flatnonzero(~used)[:: max(1, (~used).sum() // count)][:count]


@pytest.mark.parametrize("model", ["cubic", "disparity"])
def test_apply_bit_exact_and_nan_kept(fuser, c1, model):
    data = np.array(c1.depth[0] if model == "cubic" else c1.disp[0])
    t2 = c1.tiles[2]
    holes = t2.offset + _unsampled_pixels(c1, 2)
    data[holes] = np.nan  # read by no sample: the fit is unaffected, apply must keep them
    cf, _, _, after = _register(fuser, c1, [data], model, apply=True)
    assert np.isfinite(cf).all()
    want = P.apply_all(c1.tiles, data, cf[0], c1.kf, model)
    assert np.array_equal(_bits(after[0]), _bits(want))
    assert np.isnan(after[0][holes]).all() and np.isnan(after[0]).sum() == holes.size
    assert not np.array_equal(after[0], data)
    # the factor is in: the corner pixel of a tile is kf times its centre-weighted transform
    plain = P.apply_all(c1.tiles, data, cf[0], [np.ones_like(k) for k in c1.kf], model)
    assert not np.array_equal(_bits(plain), _bits(want))


def test_apply_under_the_validity_rule(fuser, c1):
    data = np.array(c1.depth[0]).reshape(-1, M.TILE, M.TILE)
    p, ys, xs = M.RECT
    data[p, ys, xs] = 0.0  # holes written as 0, rejected by lo = 0
    data = data.reshape(-1)
    fuser.set_tile_validity(0.0, INF)
    try:
        cf, _, _, after = _register(fuser, c1, [data], apply=True)
    finally:
        fuser.set_tile_validity(None, None)
    want = P.apply_all(c1.tiles, data, cf[0], c1.kf, valid=(0.0, INF))
    assert np.array_equal(_bits(after[0]), _bits(want))
    hole = after[0].reshape(-1, M.TILE, M.TILE)[p, ys, xs]
    assert np.isnan(hole).all() and np.isnan(after[0]).sum() == hole.size


# ---- 6. merge -----------------------------------------------------------------------------------
def _merge(fuser, case, emap, data, disparity=False):
    n = case.lay.ntiles
    out = torch.zeros((1, H, W), dtype=torch.int16, device=DEV)
    cf = torch.zeros((1, n, 4), dtype=torch.float32, device=DEV)
    t_tiles = _dev(data[None])
    (fuser.merge_disparity if disparity else fuser.merge)(_dev(emap[None]), t_tiles, out, ZR,
                                                          coeffs=cf)
    fuser.synchronize()
    assert np.array_equal(_bits(t_tiles.cpu().numpy()[0]), _bits(data))  # the caller's tiles stay
    return out.cpu().numpy().view(np.uint16)[0], cf.cpu().numpy()[0]


def _fuse_plain(fuser, emap, data):
    out = torch.zeros((1, H, W), dtype=torch.int16, device=DEV)
    fuser.fuse(_dev(emap[None]), _dev(data[None]), out, ZR)
    fuser.synchronize()
    return out.cpu().numpy().view(np.uint16)[0]


@pytest.mark.parametrize("model", ["cubic", "disparity"])
def test_merge(fuser, c1, model):
    emap = c1.emaps[0]
    data = c1.depth[0] if model == "cubic" else c1.disp[0]
    fuser.set_tiles(c1.lay)
    got, cf = _merge(fuser, c1, emap, data, model == "disparity")
    abcd = []
    for p in range(c1.lay.ntiles):
        xs, ys = c1.samples(0, p, data, "depth" if model == "cubic" else "disp")
        if model == "cubic":
            c, _ = P.register(xs, ys, c1.K[p])
        else:
            c, _ = P.fit(xs, ys, c1.K[p], None, 0.0, "disparity")
        abcd.append(c.astype(f32))
    assert np.array_equal(_bits(cf), _bits(np.stack(abcd)))
    xf = P.apply_all(c1.tiles, data, abcd, c1.kf, model)
    want, _ = O.solve_depth_all(emap, c1.tiles, xf, W, ZR)
    assert np.array_equal(got, want)
    assert np.array_equal(_fuse_plain(fuser, emap, xf), want)
    # and it is not what ray mode makes of the same tiles
    fuser.set_tile_depth("ray")
    try:
        ray, _ = _merge(fuser, c1, emap, data, model == "disparity")
    finally:
        fuser.set_tile_depth("planar")
    assert not np.array_equal(ray, got)


def test_merge_under_the_validity_rule(fuser, c1):
    """Holes written as 0 under lo = 0: the private copy is fused under (-inf, +inf), so pixels
    that the transform clamps to exactly 0 stay valid, and the caller's rule is back afterwards."""
    emap = c1.emaps[0]
    data = np.array(c1.depth[0]).reshape(-1, M.TILE, M.TILE)
    p, ys, xs = M.RECT
    data[p, ys, xs] = 0.0
    data = data.reshape(-1)
    nan = np.where(data > 0, data, f32(np.nan))
    fuser.set_tiles(c1.lay)
    fuser.set_tile_validity(0.0, INF)
    try:
        e, t = _dev(emap[None]), _dev(data[None])
        before = fuser.tile_valid_counts(e, t, ZR).cpu().numpy()
        got, cf = _merge(fuser, c1, emap, data)
        after = fuser.tile_valid_counts(e, t, ZR).cpu().numpy()
    finally:
        fuser.set_tile_validity(None, None)
    abcd = []
    for q in range(c1.lay.ntiles):
        xs_, ys_ = c1.samples(0, q, nan, "rect0")
        valid = ~np.isnan(xs_) & np.isfinite(ys_)
        c, _ = P.register(xs_, ys_, c1.K[q], valid)
        abcd.append(c.astype(f32))
    assert np.array_equal(_bits(cf), _bits(np.stack(abcd)))
    xf = P.apply_all(c1.tiles, data, abcd, c1.kf, valid=(0.0, INF))
    want, stats = M.masked_fuse(emap, c1.tiles, xf)
    assert np.array_equal(got, want)
    assert sum(s["dropped"] for s in stats) > 0
    # the caller's lo / hi is still in force: the zeros are still counted out
    assert np.array_equal(before, after)
    assert before[0, p, 1] == M.TILE * M.TILE - np.count_nonzero(data.reshape(-1, M.TILE, M.TILE)[p] == 0)


# ---- 7. refusals --------------------------------------------------------------------------------
def test_refusals_and_coeffless_calls(fuser, c1):
    lay, emap, data = c1.lay, c1.emaps[0], c1.depth[0]
    n = lay.ntiles
    fuser.set_tiles(lay)
    e, t = _dev(emap[None]), _dev(data[None])
    cf = torch.zeros((1, n, 4), dtype=torch.float32, device=DEV)
    cf[:, :, 2] = 1.0
    lv = O.level_dims(W, H, ZR, 1)

    def u16():
        return torch.zeros((1, H, W), dtype=torch.int16, device=DEV)

    def plane():
        return torch.zeros((lv.h, lv.w), dtype=torch.float32, device=DEV)

    def calls(coeffs):
        """name -> (call, the tensors it writes)."""
        o = {k: u16() for k in ("fuse", "check", "stitch", "smooth")}
        pl = {k: plane() for k in ("tg", "ps", "pc", "rs", "rc")}
        contrib = torch.zeros(64, dtype=torch.float32, device=DEV)
        return {
            "pf_fuse": (lambda: fuser.fuse(e, t, o["fuse"], ZR, coeffs), [o["fuse"]]),
            "pf_fuse_targets": (lambda: fuser.fuse_targets(t, coeffs, W, ZR, 1, pl["tg"]),
                                [pl["tg"]]),
            "pf_fuse_check": (lambda: fuser.fuse_check(e, t, ZR, W, coeffs=coeffs, out=o["check"]),
                              [o["check"]]),
            "pf_stitch": (lambda: fuser.stitch(t, o["stitch"], coeffs), [o["stitch"]]),
            "pf_solve_smoothing": (lambda: fuser.solve_smoothing(t, o["smooth"], ZR, coeffs),
                                   [o["smooth"]]),
            "pf_fuse_partial": (lambda: fuser.fuse_partial(t, coeffs, 0, n, W, ZR, 1, pl["ps"],
                                                           pl["pc"]), [pl["ps"], pl["pc"]]),
            "pf_fuse_partial_rows": (lambda: fuser.fuse_partial_rows(
                t, coeffs, 0, n, W, ZR, 1, lv.h0, lv.h1, pl["rs"], pl["rc"]),
                [pl["rs"], pl["rc"]]),
            "pf_fuse_multicover": (lambda: fuser.multicover(t, coeffs, 0, n, W, ZR, 1, contrib),
                                   [contrib]),
        }

    for name, (call, _) in calls(cf).items():
        with pytest.raises(panofuse.PanofuseError) as err:
            call()
        assert err.value.code == panofuse.PF_ESTATE, (name, str(err.value))
        msg = str(err.value)
        assert "pf_set_tile_depth" in msg and name + " " in msg, msg
    with pytest.raises(panofuse.PanofuseError) as err:
        fuser.register_joint(e, t, ZR, [0, 1])
    assert err.value.code == panofuse.PF_ESTATE
    assert "pf_set_tile_depth" in str(err.value) and "pf_register_joint" in str(err.value)

    # without coefficients they run, and give what ray mode gives
    planar = calls(None)
    for name, (call, outs) in planar.items():
        call()
    fuser.synchronize()
    fuser.set_tile_depth("ray")
    try:
        ray = calls(None)
        for name, (call, outs) in ray.items():
            call()
        fuser.register_joint(e, t, ZR, [0, 1])
        fuser.synchronize()
    finally:
        fuser.set_tile_depth("planar")
    for name in planar:
        for a, b in zip(planar[name][1], ray[name][1]):
            if a.dtype == torch.float32:  # bits: the targets carry NaN markers
                a, b = a.view(torch.int32), b.view(torch.int32)
            assert torch.equal(a, b), name
    assert int(planar["pf_fuse"][1][0].count_nonzero()) > 0


# ---- 8. the default path ------------------------------------------------------------------------
def test_ray_after_planar_is_the_default_path(fuser):
    g = np.load(GOLDEN)
    emap = (g["emap_u16"].astype(f32) / f32(65535.0)).astype(f32)
    data = (g["tiles_u8"].astype(f32) / f32(255.0)).astype(f32)
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
    on = run(fuser)  # planar
    fuser.set_tile_depth("ray")
    try:
        got = run(fuser)
    finally:
        fuser.set_tile_depth("planar")
    fresh = panofuse.Fuser(0)
    fresh.set_tiles(lay)
    ref = run(fresh)
    fresh.close()
    assert np.array_equal(got[0], g["out_u16"]) and np.array_equal(got[1], g["abcd"])
    assert np.array_equal(ref[0], g["out_u16"]) and np.array_equal(ref[1], g["abcd"])
    assert {k: v[2] for k, v in got[2].items()} == {k: v[2] for k, v in ref[2].items()}
    # planar: one more launch in the register stage (apply into the copy), another result
    assert on[2]["register"][2] == ref[2]["register"][2] + 1
    assert not np.array_equal(on[1], g["abcd"]) and not np.array_equal(on[0], g["out_u16"])
