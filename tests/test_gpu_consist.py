"""The overlap-consistent registration on the GPU (pf_overlap_pairs / _table / _stats,
pf_register_consistent; csrc/pf_consist.hip) against its CPU restatement (tests/consist_ref.py).

The pair table is held to an independent fp64 projection away from the window edges and the pixel
boundaries; everything downstream is bit for bit against the restatement fed with the device's own
table: the coefficients and the summary for lambda in {0, 1, 4}, the LDS and global-workspace
forms of the solve, batches, the overlap statistics, apply, the refusals, a singular panorama, and
the default path left as it was.

Shapes (small: a few seconds each): C1 with 64 x 48 tiles over a 128 x 64 baseline (three
panoramas), LeReS 64 x 48 and MiDaS 40 x 30 tiles, the mixed tile sizes and the 3-channel tiles of
tests/tile_shapes.py, and band_layout(6, 4, 64, 48, 3, 12), whose 96 unknowns do not fit the LDS
form of the solve.
"""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import consist_ref as CR  # noqa: E402
import panofuse  # noqa: E402
import pf_layouts as PL  # noqa: E402
import pf_synth  # noqa: E402
import pyoracle as O  # noqa: E402
import tile_shapes as TS  # noqa: E402

ZR = PL.ZENITH_RANGE
DEV = "cuda:0"
EW, EH, OW, OH = 128, 64, 512, 256
DELTA = 1e-5
f32 = np.float32
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
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same(got, want):
    """Bit equality, any NaN equal to any NaN."""
    got, want = np.asarray(got), np.asarray(want)
    nan = np.isnan(want)
    return (np.array_equal(np.isnan(got), nan)
            and np.array_equal(_bits(got[~nan]), _bits(want[~nan])))


def _tone(z, p):
    return ((0.8 + 0.05 * (p % 3)) * z.astype(np.float64) ** (1.1 - 0.05 * (p % 2)) + 0.03
            ).astype(f32)


class Case:
    """A layout with `nb` different panoramas of per-tile toned tiles over a blurred baseline, the
    device's pair table (fetched once) and the restatement's sums per panorama (made once)."""

    def __init__(self, lay, channels=1, nb=1, seed0=0):
        self.lay, self.channels, self.nb = lay, channels, nb
        self.tiles, total = O.make_tiles(lay, channels=channels)
        one, n1 = O.make_tiles(lay)
        self.off = [t.offset for t in self.tiles]
        self.emaps, self.data = [], []
        for b in range(nb):
            seeds = pf_synth.seeds_for(1, 20261020 + 977 * (seed0 + b))
            self.emaps.append(pf_synth.baseline_emap(seeds, EW, EH)[0].numpy())
            gt = pf_synth.scene_depth(seeds, OW, OH)[0].numpy()
            ray = O.warp_depth(gt, one, n1, O.responses(pf_synth.responses(seeds, lay.ntiles)))
            d = np.empty_like(ray)
            for p, t in enumerate(one):
                s = slice(t.offset, t.offset + t.width * t.height)
                d[s] = _tone(ray[s], p)
            self.data.append(TS.interleave(d, channels) if channels > 1 else d)
        assert self.data[0].size == total
        self._table = None
        self._sums = {}

    def table(self, fuser):
        if self._table is None:
            fuser.set_tiles(self.lay, channels=self.channels)
            pairs, index = fuser.overlap_table(ZR)
            fuser.synchronize()
            self._table = (pairs.cpu().numpy(), index.cpu().numpy())
        return self._table

    def sums(self, fuser, b, data=None, key=None):
        """(D, Pm, values) of panorama b (or of `data` under `key`) with the device's table."""
        k = (b, key)
        if k not in self._sums:
            d = self.data[b] if data is None else data
            pairs, index = self.table(fuser)
            D = [CR.data_sums(*O.reg_samples(t, d, self.emaps[b], ZR)[:2]) for t in self.tiles]
            values = CR.pair_values(self.off, d, pairs, index)
            self._sums[k] = (D, [CR.pair_sums(vp, vq) for vp, vq in values], values)
        return self._sums[k]


_CASES = {}


def case(name):
    if name not in _CASES:
        if name == "c1":
            lay = PL.config_layout("C1")
            lay.tile_w[:], lay.tile_h[:] = 64, 48
            _CASES[name] = Case(lay, nb=3)
        elif name == "leres":
            _CASES[name] = Case(PL.leres_layout(64, 48), seed0=3)
        elif name == "midas":
            _CASES[name] = Case(PL.midas_layout(40, 30), seed0=4)
        elif name == "mixed":
            _CASES[name] = Case(TS.layout_with(TS.MIXED_SIZES), seed0=5)
        elif name == "chan3":
            _CASES[name] = Case(PL.leres_layout(64, 48), channels=3, seed0=6)
        elif name == "band6x4":
            _CASES[name] = Case(PL.band_layout(6, 4, 64, 48, 3, 12), seed0=7)
        else:
            raise ValueError(name)
    return _CASES[name]


ALL = ["c1", "leres", "midas", "mixed", "chan3", "band6x4"]


def _consistent(fuser, c, datas, lam, first=0, apply=False):
    """register_consistent on panoramas first.. of the case: (coeffs, coeffs64, summary, tiles)."""
    B, n = len(datas), c.lay.ntiles
    fuser.set_tiles(c.lay, channels=c.channels)
    e, t = _dev(np.stack(c.emaps[first:first + B])), _dev(np.stack(datas))
    cf = torch.full((B, n, 4), -7.0, dtype=torch.float32, device=DEV)
    c64 = torch.full((B, n, 4), -7.0, dtype=torch.float64, device=DEV)
    sm = torch.full((B, 4), -7.0, dtype=torch.float64, device=DEV)
    fuser.register_consistent(e, t, ZR, lam=lam, apply=apply, coeffs=cf, coeffs64=c64, summary=sm)
    fuser.synchronize()
    return cf.cpu().numpy(), c64.cpu().numpy(), sm.cpu().numpy(), t.cpu().numpy()


# ---- 1. the pair table --------------------------------------------------------------------------
def _near_integer(v, tol):
    return np.abs(v - np.rint(v)) <= tol


@pytest.mark.parametrize("name", ALL)
def test_pair_table_against_the_fp64_projection(fuser, name):
    c = case(name)
    lay, ch = c.lay, c.channels
    pairs, index = c.table(fuser)
    npairs, nsamp = fuser.overlap_pairs(ZR)
    assert (npairs, nsamp) == (len(pairs), len(index)) and npairs > 0
    keys = [(int(a), int(b)) for a, b in pairs[:, :2]]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    assert all(a != b for a, b in keys)
    assert np.array_equal(pairs[:, 2], np.concatenate([[0], np.cumsum(pairs[:, 3])[:-1]]))
    assert pairs[:, 3].min() > 0 and int(pairs[:, 3].sum()) == nsamp
    for p in range(lay.ntiles):  # every element lies inside its tile
        w, h = int(lay.tile_w[p]), int(lay.tile_h[p])
        for col, sel in ((0, pairs[:, 0] == p), (1, pairs[:, 1] == p)):
            for _, _, first, count in pairs[sel]:
                e = index[first:first + count, col]
                assert e.min() >= 0 and e.max() < w * h * ch and np.all(e % ch == 0)

    proj = CR.projections64(lay, ZR)
    have = {k: i for i, k in enumerate(keys)}
    unpinned = 0
    for p in range(lay.ntiles):
        wp, hp = int(lay.tile_w[p]), int(lay.tile_h[p])
        xp, yp, _ = proj[(p, p)]
        xp, yp = np.clip(xp, 0.0, 1.0), np.clip(yp, 0.0, 1.0)
        ep = CR.elem64(xp, yp, wp, hp, ch)
        p_pinned = ~(_near_integer(xp * (wp - 1), DELTA * wp) | _near_integer(yp * (hp - 1), DELTA * hp))
        for q in range(lay.ntiles):
            if q == p:
                continue
            wq, hq = int(lay.tile_w[q]), int(lay.tile_h[q])
            x, y, den = proj[(p, q)]
            must = CR.inside64(x, y, den, DELTA, 1 - DELTA)
            never = ~CR.inside64(x, y, den, -DELTA, 1 + DELTA)
            free = ~must & ~never
            count = int(pairs[have[(p, q)], 3]) if (p, q) in have else 0
            assert must.sum() <= count <= must.sum() + free.sum(), (p, q)
            unpinned += int(free.sum())
            if count == 0:
                continue
            first = int(pairs[have[(p, q)], 2])
            got = index[first:first + count]
            with np.errstate(invalid="ignore"):
                pinned = must & p_pinned & ~(_near_integer(x * (wq - 1), DELTA * wq)
                                             | _near_integer(y * (hq - 1), DELTA * hq))
            unpinned += int((must & ~pinned).sum())
            want = np.stack([ep[pinned], CR.elem64(np.where(pinned, x, 0.0), np.where(pinned, y, 0.0),
                                                   wq, hq, ch)[pinned]], 1)
            if not free.any():  # the kept samples are exactly `must`, in sample order
                assert np.array_equal(got[pinned[must]], want), (p, q)
            else:  # near an edge: every pinned row is there
                grows, gn = np.unique(got, axis=0, return_counts=True)
                lookup = {tuple(r): k for r, k in zip(grows.tolist(), gn.tolist())}
                wrows, wn = np.unique(want, axis=0, return_counts=True)
                assert all(lookup.get(tuple(r), 0) >= k for r, k in zip(wrows.tolist(), wn.tolist())), (p, q)
    share = unpinned / nsamp
    print(f"{name}: {npairs} pairs, {nsamp} pair samples, unpinned {unpinned} ({100 * share:.2f} %)")
    assert share <= 0.02


# ---- 2. pf_register_consistent ------------------------------------------------------------------
@pytest.mark.parametrize("lam", [0.0, 1.0, 4.0])
@pytest.mark.parametrize("name", ALL)
def test_register_consistent_bit_exact(fuser, name, lam):
    c = case(name)
    pairs, _ = c.table(fuser)
    cf, c64, sm, after = _consistent(fuser, c, c.data[:1], lam)
    assert np.array_equal(_bits(after[0]), _bits(c.data[0]))  # apply=False leaves the tiles
    D, Pm, _ = c.sums(fuser, 0)
    want, wsm = CR.register(D, Pm, pairs, lam)
    print(f"{name} lambda {lam}: summary gpu {sm[0]} ref {wsm}")
    assert wsm[3] == 0.0
    assert _same(c64[0], want)
    assert _same(cf[0], want.astype(f32))
    assert _same(sm[0], wsm)
    if lam == 0.0:  # the independent least squares: pf_register's normal-equation minimiser
        fuser.set_solver("normal")
        try:
            r64 = torch.zeros((1, c.lay.ntiles, 4), dtype=torch.float64, device=DEV)
            fuser.register(_dev(c.emaps[0][None]), _dev(c.data[0][None]), ZR, apply=False,
                           coeffs64=r64)
            fuser.synchronize()
        finally:
            fuser.set_solver("lm")
        r64 = r64.cpu().numpy()[0]
        rel = np.abs(c64[0] - r64).max() / np.abs(r64).max()
        print(f"   against pf_register (normal): max rel {rel:.3g}")
        assert rel < 1e-5


def test_batch_gives_the_bits_of_the_single_runs(fuser):
    c = case("c1")
    pairs, _ = c.table(fuser)
    cf, c64, sm, _ = _consistent(fuser, c, c.data, 1.0)
    for b in range(3):
        s_cf, s_c64, s_sm, _ = _consistent(fuser, c, c.data[b:b + 1], 1.0, first=b)
        assert _same(c64[b], s_c64[0]) and _same(cf[b], s_cf[0]) and _same(sm[b], s_sm[0])
        D, Pm, _ = c.sums(fuser, b)
        want, wsm = CR.register(D, Pm, pairs, 1.0)
        assert _same(c64[b], want) and _same(sm[b], wsm)
    assert not np.array_equal(c64[0], c64[1]) and not np.array_equal(c64[1], c64[2])


@pytest.mark.parametrize("name", ["c1", "leres"])
def test_workspace_form_gives_the_lds_forms_bits(fuser, name):
    c = case(name)
    lds = _consistent(fuser, c, c.data[:1], 4.0)
    os.environ["PF_CONSIST_WORKSPACE"] = "1"
    try:
        ws = _consistent(fuser, c, c.data[:1], 4.0)
    finally:
        del os.environ["PF_CONSIST_WORKSPACE"]
    for a, b in zip(lds[:3], ws[:3]):
        assert _same(a, b)
    assert np.isfinite(ws[1]).all()


# ---- 3. pf_overlap_stats ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c1", "chan3", "mixed"])
def test_overlap_stats_bit_exact(fuser, name):
    c = case(name)
    pairs, index = c.table(fuser)
    cf, _, _, _ = _consistent(fuser, c, c.data[:1], 1.0)
    _, _, values = c.sums(fuser, 0)
    t = _dev(c.data[0][None])
    raw = fuser.overlap_stats(t, ZR).cpu().numpy()[0]
    con = fuser.overlap_stats(t, ZR, coeffs=_dev(cf)).cpu().numpy()[0]
    assert _same(raw, CR.overlap_stats(values, pairs))
    assert _same(con, CR.overlap_stats(values, pairs, cf[0]))
    assert np.array_equal(raw[:, 0], pairs[:, 3]) and not raw[:, 4].any()
    ind, _, _, _ = _consistent(fuser, c, c.data[:1], 0.0)
    before = CR.overlap_rms(fuser.overlap_stats(t, ZR, coeffs=_dev(ind)).cpu().numpy())
    after = CR.overlap_rms(con)
    print(f"{name}: overlap rms raw {CR.overlap_rms(raw):.5f}, independent {before:.5f}, "
          f"consistent (lambda 1) {after:.5f}")
    assert after <= before


def test_overlap_stats_counts_planted_nans_apart(fuser):
    c = case("c1")
    pairs, index = c.table(fuser)
    fuser.set_tiles(c.lay)
    data = c.data[0].copy()
    p, q, first, count = pairs[0].tolist()
    holes = np.unique(index[first:first + count, 0])[:5]
    data[c.off[p] + holes] = np.nan
    values = CR.pair_values(c.off, data, pairs, index)
    got = fuser.overlap_stats(_dev(data[None]), ZR).cpu().numpy()[0]
    want = CR.overlap_stats(values, pairs)
    assert _same(got, want)
    assert got[0, 4] > 0 and got[0, 0] + got[0, 4] == count
    assert np.isfinite(got[:, :4]).all()  # the NaNs show in the fifth entry only
    clean = fuser.overlap_stats(_dev(c.data[0][None]), ZR).cpu().numpy()[0]
    touched = got[:, 4] > 0
    assert touched.any() and np.array_equal(_bits(got[~touched]), _bits(clean[~touched]))


# ---- 4. apply -----------------------------------------------------------------------------------
def test_apply_is_pf_registers_transform(fuser):
    c = case("chan3")
    cf, _, _, after = _consistent(fuser, c, c.data[:1], 1.0, apply=True)
    want = c.data[0].copy()
    for p, t in enumerate(c.tiles):
        O.depth_to_depth(t, want, cf[0, p])
    assert np.array_equal(_bits(after[0]), _bits(want))
    assert not np.array_equal(after[0], c.data[0]) and TS.fill_kept(after[0])


# ---- 5. refusals --------------------------------------------------------------------------------
def test_refusals(fuser):
    c = case("c1")
    fuser.set_tiles(c.lay)
    e, t = _dev(c.emaps[0][None]), _dev(c.data[0][None])
    st = torch.zeros((1, fuser.overlap_pairs(ZR)[0], 5), dtype=torch.float64, device=DEV)
    calls = {
        "pf_overlap_pairs": lambda: fuser.overlap_pairs(ZR),
        # the entry itself: the wrapper asks pf_overlap_pairs for the size first
        "pf_overlap_stats": lambda: fuser._check(fuser.L.pf_overlap_stats(
            fuser.h, panofuse._ptr(t), None, 1, float(ZR[0]), float(ZR[1]), panofuse._ptr(st))),
        "pf_register_consistent": lambda: fuser.register_consistent(e, t, ZR, apply=False),
    }
    modes = [
        ("pf_set_tile_validity", lambda: fuser.set_tile_validity(0.0, 1.0),
         lambda: fuser.set_tile_validity(None, None)),
        ("pf_set_register_loss", lambda: fuser.set_register_loss("huber", 0.02),
         lambda: fuser.set_register_loss(None)),
        ("pf_set_tile_depth", lambda: fuser.set_tile_depth("planar"),
         lambda: fuser.set_tile_depth("ray")),
    ]
    for setter, on, off in modes:
        on()
        try:
            for name, call in calls.items():
                with pytest.raises(panofuse.PanofuseError) as err:
                    call()
                assert err.value.code == panofuse.PF_ESTATE, (setter, name)
                assert setter in str(err.value) and name in str(err.value), str(err.value)
            with pytest.raises(panofuse.PanofuseError) as err:  # before its buffers are made
                fuser.overlap_table(ZR)
            assert err.value.code == panofuse.PF_ESTATE
        finally:
            off()
        for call in calls.values():  # and they run again once the mode is off
            call()
        fuser.synchronize()
    for lam in (-1.0, float("nan"), float("inf")):
        with pytest.raises(panofuse.PanofuseError) as err:
            fuser.register_consistent(e, t, ZR, lam=lam, apply=False)
        assert err.value.code == panofuse.PF_EINVAL and "lambda" in str(err.value)
    fuser.register_consistent(e, t, ZR, lam=0.5, apply=False)
    fuser.synchronize()


# ---- 6. a singular panorama ---------------------------------------------------------------------
def test_singular_panorama_gets_nans_and_status_1(fuser):
    c = case("c1")
    pairs, _ = c.table(fuser)
    flat = c.data[0].copy()
    for p in (1, 4):  # two constant tiles: their 4 x 4 blocks have rank 1
        t = c.tiles[p]
        flat[t.offset:t.offset + t.width * t.height] = f32(0.5)
    D, Pm, _ = c.sums(fuser, 0, flat, "flat")
    want, wsm = CR.register(D, Pm, pairs, 1.0)
    assert wsm[3] == 1.0 and np.isnan(want).all()
    e = _dev(np.stack([c.emaps[0], c.emaps[1]]))
    t = _dev(np.stack([flat, c.data[1]]))
    cf = torch.zeros((2, 6, 4), dtype=torch.float32, device=DEV)
    c64 = torch.zeros((2, 6, 4), dtype=torch.float64, device=DEV)
    sm = torch.zeros((2, 4), dtype=torch.float64, device=DEV)
    fuser.set_tiles(c.lay)
    fuser.register_consistent(e, t, ZR, lam=1.0, apply=False, coeffs=cf, coeffs64=c64, summary=sm)
    fuser.synchronize()
    cf, c64, sm = cf.cpu().numpy(), c64.cpu().numpy(), sm.cpu().numpy()
    assert np.isnan(c64[0]).all() and np.isnan(cf[0]).all()
    assert _same(sm[0], wsm) and sm[0, 3] == 1.0 and sm[0, 2] == pairs[:, 3].sum()
    D1, P1, _ = c.sums(fuser, 1)
    w1, s1 = CR.register(D1, P1, pairs, 1.0)
    assert _same(c64[1], w1) and _same(sm[1], s1) and sm[1, 3] == 0.0


# ---- 7. the default path ------------------------------------------------------------------------
def test_default_path_after_the_new_calls(fuser):
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
    e, t = _dev(emap[None]), _dev(data.reshape(1, -1))
    fuser.profile(True)
    fuser.register_consistent(e, t, ZR, lam=1.0, apply=False)
    fuser.overlap_stats(t, ZR)
    fuser.synchronize()
    mine = fuser.profile_read()
    fuser.profile(False)
    assert mine["register"][2] == 3 + 1  # moments, pair moments, solve; the statistics
    assert all(v[2] == 0 for k, v in mine.items() if k != "register")
    got = run(fuser)
    fresh = panofuse.Fuser(0)
    fresh.set_tiles(lay)
    ref = run(fresh)
    fresh.close()
    assert np.array_equal(got[0], g["out_u16"]) and np.array_equal(got[1], g["abcd"])
    assert np.array_equal(ref[0], g["out_u16"]) and np.array_equal(ref[1], g["abcd"])
    assert {k: v[2] for k, v in got[2].items()} == {k: v[2] for k, v in ref[2].items()}
