"""Per-pixel weights for disparity tiles (pf_tile_range_weights, pf_register_disparity_weighted,
pf_merge_disparity_weighted) on the GPU, bit for bit against tests/disp_weight_ref.py (which
tests/test_disp_weight_ref.py proves against disp_ref.py).

Shapes: C1 (6 tiles of 256^2, 7,865 samples each, 512x256 output), the one-tile 121 x 121 grid
above the resident capacity, 500x248 of test_fuse_shapes.SHAPES for the fusion, and the mixed-size
and three-channel layouts of tests/mask_shapes.py for the range weights.  Every reference is
computed once per process and shared.
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import disp_weight_cases as CS  # noqa: E402
import disp_weight_ref as R  # noqa: E402
import mask_ref as M  # noqa: E402
import mask_shapes as MS  # noqa: E402
import panofuse  # noqa: E402
import planar_ref as P  # noqa: E402
import pyoracle as O  # noqa: E402
import weight_ref as WR  # noqa: E402
from test_oracle import GOLDEN  # noqa: E402

f32 = np.float32
ZR = CS.ZR
DEV = "cuda:0"
INF = float("inf")
RESIDENT = 8192  # kDispResident of csrc/pf_lm.hpp
NS_C1 = 7865


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a)).to(DEV)  # a copy: the inputs are read-only


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(got, ref):
    """Equal bit for bit where ref is not NaN, NaN where it is."""
    got, ref = np.asarray(got), np.asarray(ref)
    nan = np.isnan(ref)
    return bool(np.array_equal(np.isnan(got), nan)
                and np.array_equal(_bits(got[~nan]), _bits(ref[~nan])))


def _fuser(lay, channels=1):
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected on a host without a GPU")
    fz = panofuse.Fuser(0)
    fz.set_tiles(lay, channels)
    return fz


@pytest.fixture(scope="module")
def fuser():
    return _fuser(CS.c1(0)[0])


def _register_w(fz, emaps, datas, w, apply=False):
    """(coeffs32 [B][n][4], coeffs64, summary [B][n][6], tiles after the call)."""
    datas = np.atleast_2d(datas)
    B, n = datas.shape[0], fz.layout.ntiles
    e = _dev(np.stack(emaps) if isinstance(emaps, list) else np.broadcast_to(
        emaps, (B,) + np.shape(emaps)))
    t = _dev(datas)
    c32 = torch.full((B, n, 4), -7.0, dtype=torch.float32, device=DEV)
    c64 = torch.full((B, n, 4), -7.0, dtype=torch.float64, device=DEV)
    sm = torch.full((B, n, 6), -7.0, dtype=torch.float64, device=DEV)
    fz.register_disparity_weighted(e, t, _dev(w), ZR, apply=apply, coeffs=c32, coeffs64=c64,
                                   summary=sm)
    fz.synchronize()
    return c32.cpu().numpy(), c64.cpu().numpy(), sm.cpu().numpy(), t.cpu().numpy()


def _merge_w(fz, emap, data, w, out_w=512):
    data = np.atleast_2d(data)
    B = data.shape[0]
    t = _dev(data)
    out = torch.zeros((B, out_w // 2, out_w), dtype=torch.int16, device=DEV)
    cf = torch.full((B, fz.layout.ntiles, 4), -7.0, dtype=torch.float32, device=DEV)
    fz.merge_disparity_weighted(_dev(np.broadcast_to(emap, (B,) + np.shape(emap))), t, _dev(w),
                                out, ZR, coeffs=cf)
    fz.synchronize()
    assert np.array_equal(_bits(t.cpu().numpy()), _bits(data)), "the caller's tiles stay"
    return out.cpu().numpy().view(np.uint16), cf.cpu().numpy()


def _check_register(fz, tiles, emap, data, w, kfs=None, floor=R.MIN_USED):
    """register_disparity_weighted of one panorama against the restatement: coeffs, coeffs64 and
    all six summary entries.  Returns (reference coeffs64, reference summary)."""
    r64, rsum = R.register(tiles, data, w, emap, kfs=kfs)
    assert (rsum[:, 4] >= floor).all(), "every tile keeps enough used samples"
    c32, c64, sm, after = _register_w(fz, emap, data, w)
    assert np.array_equal(_bits(after[0]), _bits(np.asarray(data))), "apply = 0 leaves the tiles"
    for p in range(len(tiles)):
        print(f"tile {p}: gpu {c64[0, p]} ref {r64[p]} summary {sm[0, p]} ref {rsum[p]}")
    assert _same(c64[0], r64) and _same(c32[0], r64.astype(f32))
    assert _same(sm[0], rsum)
    return r64, rsum


# ---- the weight sets ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def c1_tent():
    w = WR.tent(CS.c1(0)[1])
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def c1_odd():
    """The field with odd weights under sampled elements of every tile: NaN, -1, +inf, -0 (not
    usable), a denormal and a huge one (usable)."""
    _, tiles, emap, _ = CS.c1(0)
    w = np.array(CS.c1_field())
    odd = np.array([np.nan, -1.0, np.inf, -0.0, 1e-40, 3e38], f32)
    for t in tiles:
        el = np.unique(WR.sample_elements(t, emap))
        el = el[w[t.offset + el] > 0]
        w[t.offset + el[::el.size // 60][:60]] = np.tile(odd, 10)
    w.setflags(write=False)
    return w


# ---- 1. C1: coefficients and the six summary entries -------------------------------------------
def test_ones_is_register_disparity(fuser):
    """Every weight 1.0f: every bit of coeffs, coeffs64 and the first four summary entries is
    pf_register_disparity's on the same context."""
    lay, tiles, emap, disp = CS.c1(0)
    ones = np.ones(disp.size, f32)
    c32, c64, sm, after = _register_w(fuser, emap, disp, ones, apply=True)
    t = _dev(disp[None])
    p32 = torch.zeros((1, 6, 4), dtype=torch.float32, device=DEV)
    p64 = torch.zeros((1, 6, 4), dtype=torch.float64, device=DEV)
    psm = torch.zeros((1, 6, 4), dtype=torch.float64, device=DEV)
    fuser.register_disparity(_dev(emap[None]), t, ZR, apply=True, coeffs=p32, coeffs64=p64,
                             summary=psm)
    fuser.synchronize()
    assert np.isfinite(c64).all() and (c64[0, :, 2] == 1.0).all()
    assert np.array_equal(_bits(c32), _bits(p32.cpu().numpy()))
    assert np.array_equal(_bits(c64), _bits(p64.cpu().numpy()))
    assert np.array_equal(_bits(sm[..., :4]), _bits(psm.cpu().numpy()))
    assert (sm[0, :, 4] == NS_C1).all() and (sm[0, :, 5] == NS_C1).all()
    assert np.array_equal(_bits(after), _bits(t.cpu().numpy()))  # apply: the same transform
    assert not np.array_equal(after[0], disp)


@pytest.mark.parametrize("kind", ["tent", "field", "odd"])
def test_c1_weighted_registration(fuser, kind):
    lay, tiles, emap, disp = CS.c1(0)
    w = {"tent": c1_tent, "field": CS.c1_field, "odd": c1_odd}[kind]()
    r64, rsum = _check_register(fuser, tiles, emap, disp, w)
    assert np.isfinite(r64).all()
    if kind == "field":  # the exact-zero rectangle switches samples of tile 0 off
        assert rsum[0, 4] < NS_C1 and (rsum[1:, 4] == NS_C1).all()
    if kind == "odd":
        assert (rsum[:, 4] < NS_C1).all()
    if kind == "tent":
        plain, _ = R.register(tiles, disp, np.ones(disp.size, f32), emap)
        assert not np.array_equal(plain, r64), "the weights must matter"


# ---- 2. above the resident capacity -------------------------------------------------------------
def test_grid_above_resident_capacity():
    """121 x 121 samples: those past the capacity are gathered again in every pass and take their
    weight too.  The weights switch samples off on both sides of the capacity boundary."""
    lay, tiles, emap, disp = CS.wide()
    el = WR.sample_elements(tiles[0], emap)
    assert el.size > RESIDENT and el.size % 256 != 0
    w = np.array(CS.smooth_field(tiles, 11))
    off = np.r_[np.arange(RESIDENT - 700, RESIDENT + 900, 3), np.arange(40, 4000, 17),
                np.arange(RESIDENT + 2000, el.size, 5)]
    w[el[off]] = 0.0
    _, _, W, used, _ = R.tile_samples(tiles[0], disp, w, emap)
    assert (~used[:RESIDENT]).any() and (~used[RESIDENT:]).any()
    assert used[:RESIDENT].any() and used[RESIDENT:].any()
    _check_register(_fuser(lay), tiles, emap, disp, w)


# ---- 3. batches ---------------------------------------------------------------------------------
def test_batch_of_three(fuser):
    """Three panoramas against their single runs, with one weight set and with three; panorama 1
    carries a NaN tile pixel under weight 1, which only its own fit may see."""
    lay, tiles, _, _ = CS.c1(0)
    emaps = [CS.c1(s)[2] for s in range(3)]
    disps = [np.array(CS.c1(s)[3]) for s in range(3)]
    el = WR.sample_elements(tiles[2], emaps[1])
    vals, counts = np.unique(el, return_counts=True)
    at = int(vals[counts == 1][100])
    disps[1][tiles[2].offset + at] = np.nan
    ones = np.ones(disps[0].size, f32)
    sets = np.stack([np.asarray(CS.c1_field()), c1_tent(), ones])
    assert sets[1][tiles[2].offset + at] > 0 and CS.c1_field()[tiles[2].offset + at] > 0
    for w in (np.asarray(CS.c1_field()), sets):
        c32, c64, sm, _ = _register_w(fuser, emaps, np.stack(disps), w)
        for b in range(3):
            wb = w if w.ndim == 1 else w[b]
            s32, s64, ssm, _ = _register_w(fuser, emaps[b], disps[b], wb)
            assert _same(c64[b], s64[0]) and _same(c32[b], s32[0]) and _same(sm[b], ssm[0]), b
        assert np.isfinite(c64).all()
        assert not np.array_equal(c64[0], c64[1]) and not np.array_equal(c64[1], c64[2])
    # the NaN pixel costs panorama 1's tile 2 exactly one sample (wbatch = 3: the tent there)
    clean = np.array(CS.c1(1)[3])
    _, _, csm, _ = _register_w(fuser, emaps[1], clean, sets[1])
    assert sm[1, 2, 4] == csm[0, 2, 4] - 1 == NS_C1 - 1
    assert sm[2, 2, 4] == NS_C1 and sm[2, 2, 5] == NS_C1
    r64, rsum = R.register(tiles, disps[1], sets[1], emaps[1])
    assert _same(c64[1], r64) and _same(sm[1], rsum)


# ---- 4. tiles with exactly 3, 2 and 0 used samples ---------------------------------------------
def test_few_used_samples(fuser):
    lay, tiles, emap, disp = CS.c1(0)
    w = np.array(CS.c1_field())

    def keep(p, k):
        t = tiles[p]
        vals, counts = np.unique(WR.sample_elements(t, emap), return_counts=True)
        once = vals[counts == 1]
        chosen = once[np.linspace(0, once.size - 1, k + 2).astype(int)[1:k + 1]]
        kept = w[t.offset + chosen].copy()
        assert np.unique(chosen).size == k and (kept > 0).all()
        w[t.offset:t.offset + t.width * t.height] = 0.0
        w[t.offset + chosen] = kept

    keep(0, 3)
    keep(1, 2)
    keep(2, 0)
    r64, rsum = _check_register(fuser, tiles, emap, disp, w, floor=0)
    assert list(rsum[:3, 4]) == [3, 2, 0] and (rsum[3:, 4] == NS_C1).all()
    assert np.isfinite(r64[0]).all()
    assert np.isnan(r64[1:3]).all() and list(rsum[1:3, 3]) == [5, 5]
    assert np.isnan(rsum[1:3, :2]).all() and list(rsum[1:3, 2]) == [0, 0]
    # the other tiles are the field's own fits
    f64, fsum = R.register(tiles, disp, CS.c1_field(), emap)
    assert np.array_equal(_bits(r64[3:]), _bits(f64[3:]))
    assert np.array_equal(_bits(rsum[3:]), _bits(fsum[3:]))
    # the failed tiles are written as quiet NaNs
    c32, c64, _, _ = _register_w(fuser, emap, disp, w)
    assert (_bits(c64[0, 1:3]) == 0x7FF8000000000000).all()
    assert (_bits(c32[0, 1:3]) == 0x7FC00000).all()


# ---- 5. the merge -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def c1_merge_ref(kind):
    _, tiles, emap, disp = CS.c1(0)
    w, d = {"field": (CS.c1_field(), disp), "sky": (None, CS.sky(tiles, disp))}[kind]
    if w is None:
        w = R.range_weights(d, 0.0, INF)
    return R.merge(emap, tiles, d, w), w, d


def test_merge_c1(fuser):
    _, tiles, emap, disp = CS.c1(0)
    (ref, rabcd), w, _ = c1_merge_ref("field")
    assert np.isfinite(rabcd).all()
    out, cf = _merge_w(fuser, emap, disp, w)
    assert np.array_equal(_bits(cf[0]), _bits(rabcd))
    assert np.array_equal(out[0], ref)
    # against the unweighted merge: the weights must matter
    plain = torch.zeros((1, 256, 512), dtype=torch.int16, device=DEV)
    fuser.merge_disparity(_dev(emap[None]), _dev(disp[None]), plain, ZR)
    fuser.synchronize()
    assert (plain.cpu().numpy().view(np.uint16)[0] != out[0]).any()


def test_merge_sky_with_range_weights(fuser):
    """Tiles whose top rows are disparity 0 ("sky"): weights from range_weights(0, inf) on the
    device switch the block off, in the fit and in the fusion."""
    _, tiles, emap, _ = CS.c1(0)
    (ref, rabcd), w, d = c1_merge_ref("sky")
    got_w = fuser.range_weights(_dev(d[None]), 0.0, INF)
    fuser.synchronize()
    assert np.array_equal(_bits(got_w.cpu().numpy()[0]), _bits(w))
    assert 0 < w.sum() < w.size and np.isfinite(rabcd).all()
    B = 1
    out = torch.zeros((B, 256, 512), dtype=torch.int16, device=DEV)
    cf = torch.zeros((B, 6, 4), dtype=torch.float32, device=DEV)
    fuser.merge_disparity_weighted(_dev(emap[None]), _dev(d[None]), got_w, out, ZR, coeffs=cf)
    fuser.synchronize()
    assert np.array_equal(_bits(cf.cpu().numpy()[0]), _bits(rabcd))
    assert np.array_equal(out.cpu().numpy().view(np.uint16)[0], ref)


def _zero_tile_field(tiles):
    """The C1 field with weight 0 on every pixel of tile M.ALL_TILE."""
    w = np.array(CS.c1_field())
    t = tiles[M.ALL_TILE]
    w[t.offset:t.offset + t.width * t.height] = 0.0
    return w


def test_merge_with_an_all_zero_tile(fuser):
    """Tile 4 has weight 0 everywhere: NaN coefficients, an all-NaN transformed copy, and the
    pixels only it covers keep the baseline: there the result is that of a merge in which no tile
    counts at all (every weight 0).  The pixels are those of the finest level that lie in tile
    4's box and in no other, 8 pixels or more from the region's rim (two coarsest-level pixels,
    the reach of the upsampling's interpolation)."""
    _, tiles, emap, disp = CS.c1(0)
    w = _zero_tile_field(tiles)
    ref, rabcd = R.merge(emap, tiles, disp, w)
    assert np.isnan(rabcd[M.ALL_TILE]).all() and np.isfinite(np.delete(rabcd, M.ALL_TILE, 0)).all()
    out, cf = _merge_w(fuser, emap, disp, w)
    assert _same(cf[0], rabcd)
    assert np.array_equal(out[0], ref)
    full, _ = c1_merge_ref("field")[0]
    assert (ref != full).any()
    lv = O.level_dims(512, 256, ZR, O.num_levels(512) - 1)
    inbox = [WR.tile_taps(tiles, p, lv)[0] for p in range(len(tiles))]
    alone = inbox[M.ALL_TILE] & ~np.any(np.delete(np.stack(inbox), M.ALL_TILE, 0), axis=0)
    for _ in range(8):  # erode by one pixel
        e = alone.copy()
        e[1:] &= alone[:-1]
        e[:-1] &= alone[1:]
        e[:, 1:] &= alone[:, :-1]
        e[:, :-1] &= alone[:, 1:]
        alone = e
    alone[:lv.h0 + 1] = False
    alone[lv.h1:] = False
    assert alone.sum() > 5000, "C1 has pixels that tile 4 covers alone"
    base, babcd = _merge_w(fuser, emap, disp, np.zeros(disp.size, f32))
    assert np.isnan(babcd).all()
    assert np.array_equal(out[0][alone], base[0][alone])
    assert (full[alone] != base[0][alone]).any(), "with its weights the tile moves those pixels"


def test_merge_at_496x248():
    """pf_merge_disparity_weighted itself at an off-power size of test_fuse_shapes.SHAPES whose
    height is out_w / 2 (a strip wider than a row; levels on other engines than 512 x 256), with
    the all-zero tile staged as NaN, against the restatement; its register stage is three
    launches and its Jacobi launches are those of pf_merge_weighted at the same size."""
    case = MS.row_case((496, 248))
    lay, tiles, _, disp = CS.c1(0)
    w = _zero_tile_field(tiles)
    ref, rabcd = R.merge(case.emap, tiles, disp, w, out_w=496)
    assert ref.shape == (248, 496) and np.isnan(rabcd[M.ALL_TILE]).all()
    assert np.isfinite(np.delete(rabcd, M.ALL_TILE, 0)).all()
    fz = _fuser(lay)
    fz.profile(True)
    out, cf = _merge_w(fz, case.emap, disp, w, out_w=496)
    launches = {k: v[2] for k, v in fz.profile_read().items()}
    assert _same(cf[0], rabcd)
    assert np.array_equal(out[0], ref)
    o2 = torch.zeros((1, 248, 496), dtype=torch.int16, device=DEV)
    fz.merge_weighted(_dev(case.emap[None]), _dev(np.asarray(case.data)[None]), _dev(w), o2, ZR)
    fz.synchronize()
    cubic = {k: v[2] for k, v in fz.profile_read().items()}
    fz.profile(False)
    assert launches["register"] == 3
    assert launches["jacobi"] == cubic["jacobi"] and launches["targets"] == cubic["targets"]


def test_fusion_at_500x248():
    """An off-power size of test_fuse_shapes.SHAPES.  The merge's height is out_w / 2, so the size
    runs as the merge's two halves: register_disparity_weighted with apply on a copy, then
    fuse_weighted on the copy without coefficients, against the restatement's two halves."""
    case = MS.row_case((500, 248))
    lay, tiles, _, disp = CS.c1(0)
    emap, w = case.emap, CS.c1_field()
    fz = _fuser(lay)
    r64, rsum = _check_register(fz, tiles, emap, disp, w)
    copy = R.transform_all(tiles, disp, r64.astype(f32))
    ref = WR.fuse(emap, tiles, copy, w, None, 500, 248)
    _, _, _, after = _register_w(fz, emap, disp, w, apply=True)
    assert _same(after[0], copy)
    out = torch.zeros((1, 248, 500), dtype=torch.int16, device=DEV)
    fz.fuse_weighted(_dev(emap[None]), _dev(after), _dev(w), out, ZR)
    fz.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint16)[0], ref)


# ---- 6. planar-depth tiles ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def planar():
    fz = _fuser(CS.c1(0)[0])
    fz.set_tile_depth("planar")
    yield fz, P.layout_kf(CS.c1(0)[0])
    fz.close()


def test_planar_register(planar):
    fz, kfs = planar
    _, tiles, emap, disp = CS.c1(0)
    r64, _ = _check_register(fz, tiles, emap, disp, CS.c1_field(), kfs=kfs)
    ray, _ = R.register(tiles, disp, CS.c1_field(), emap)
    assert np.isfinite(r64).all() and not np.array_equal(r64, ray)
    # every weight 1.0f: pf_register_disparity's planar fit on the same context
    ones = np.ones(disp.size, f32)
    c32, c64, sm, _ = _register_w(fz, emap, disp, ones)
    p64 = torch.zeros((1, 6, 4), dtype=torch.float64, device=DEV)
    psm = torch.zeros((1, 6, 4), dtype=torch.float64, device=DEV)
    fz.register_disparity(_dev(emap[None]), _dev(disp[None]), ZR, apply=False, coeffs64=p64,
                          summary=psm)
    fz.synchronize()
    assert np.array_equal(_bits(c64), _bits(p64.cpu().numpy()))
    assert np.array_equal(_bits(sm[..., :4]), _bits(psm.cpu().numpy()))


def test_planar_merge(planar):
    fz, kfs = planar
    _, tiles, emap, disp = CS.c1(0)
    w = CS.c1_field()
    ref, rabcd = R.merge(emap, tiles, disp, w, kfs=kfs)
    out, cf = _merge_w(fz, emap, disp, w)
    assert np.array_equal(_bits(cf[0]), _bits(rabcd)) and np.isfinite(rabcd).all()
    assert np.array_equal(out[0], ref)
    assert (ref != c1_merge_ref("field")[0][0]).any()


# ---- 7. range weights ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["MIXED", "LERES3"])
def test_range_weights(name):
    case = MS.layout_case(name)
    fz = _fuser(case.lay, case.channels)
    rs = np.random.RandomState(5)
    d = np.stack([np.array(case.data), np.array(case.data)])
    odd = np.array([np.nan, 0.0, -0.0, np.inf, -np.inf, 1e-40, 1.0, 0.999], f32)
    at = rs.choice(d[0].size, 4000, replace=False)
    d[0, at] = odd[rs.randint(0, odd.size, at.size)]
    d[1, at[::2]] = 0.0
    for lo, hi in ((0.0, INF), (0.0, 1.0), (0.25, 0.75), (-INF, INF)):
        out = torch.full(d.shape, -3.0, dtype=torch.float32, device=DEV)
        got = fz.range_weights(_dev(d), lo, hi, out=out)
        fz.synchronize()
        ref = R.range_weights(d, lo, hi, case.channels)
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(ref)), (lo, hi)
        assert 0 < ref.sum() < ref.size
    if case.channels == 3:
        assert not ref[:, 1::3].any() and not ref[:, 2::3].any()


# ---- 8. refusals --------------------------------------------------------------------------------
def test_refusals():
    lay, tiles, emap, disp = CS.c1(0)
    fz = _fuser(lay)
    e, t, w = _dev(emap[None]), _dev(disp[None]), _dev(c1_tent())
    out = torch.zeros((1, 256, 512), dtype=torch.int16, device=DEV)
    calls = {"pf_register_disparity_weighted":
             lambda: fz.register_disparity_weighted(e, t, w, ZR, apply=False),
             "pf_merge_disparity_weighted": lambda: fz.merge_disparity_weighted(e, t, w, out, ZR)}
    modes = [("pf_set_tile_validity", lambda: fz.set_tile_validity(-INF, INF),
              lambda: fz.set_tile_validity(None, None)),
             ("pf_set_register_loss", lambda: fz.set_register_loss("huber", 0.1),
              lambda: fz.set_register_loss(None))]
    for setter, on, off in modes:
        on()
        try:
            for entry, call in calls.items():
                with pytest.raises(panofuse.PanofuseError) as err:
                    call()
                assert err.value.code == panofuse.PF_ESTATE, (setter, entry)
                assert setter in str(err.value) and entry in str(err.value), str(err.value)
            # the state check comes before the argument checks
            with pytest.raises(panofuse.PanofuseError) as err:
                fz.register_disparity_weighted(e, t, None, ZR)
            assert err.value.code == panofuse.PF_ESTATE
            fz.range_weights(t, 0.0, INF)  # refuses nothing but bad arguments
        finally:
            off()
        for call in calls.values():  # and they run again
            call()
        fz.synchronize()
    e3, t3 = _dev(np.stack([emap] * 3)), _dev(np.stack([disp] * 3))
    out3 = torch.zeros((3, 256, 512), dtype=torch.int16, device=DEV)
    two = _dev(np.stack([c1_tent()] * 2))
    for call in (lambda: fz.register_disparity_weighted(e3, t3, None, ZR),
                 lambda: fz.merge_disparity_weighted(e3, t3, None, out3, ZR),
                 lambda: fz.register_disparity_weighted(e3, t3, two, ZR),
                 lambda: fz.merge_disparity_weighted(e3, t3, two, out3, ZR)):
        with pytest.raises(panofuse.PanofuseError) as err:
            call()
        assert err.value.code == panofuse.PF_EINVAL, str(err.value)
    with pytest.raises(ValueError):
        fz.range_weights(_dev(np.ones(5, f32)), 0.0, 1.0)


def test_layout_above_2_30_tile_elements():
    """Five tiles of 16384^2 are 5 * 2^28 > 2^30 tile elements: the merge refuses the layout
    (its gather has the per-wave form only) before anything is allocated or launched, so it is
    called through the C ABI with small stand-in buffers.  The registration takes the layout: on
    real buffers (5.4 GB of tiles, as much of weights) and with every weight 1.0f it is
    pf_register_disparity bit for bit, with the element offsets of the last tile past 2^30."""
    import pf_layouts as PL
    full = PL.band_layout(5, 1, 16384, 16384, 3, 12, "five-huge-tiles")
    fz = _fuser(full)
    assert fz.tile_elems == 5 << 28 and fz.tile_elems > 1 << 30
    emap = CS.c1(0)[2]
    e = _dev(emap[None])
    small = torch.zeros(1024, dtype=torch.float32, device=DEV)
    out = torch.zeros((1, 256, 512), dtype=torch.int16, device=DEV)
    rc = fz.L.pf_merge_disparity_weighted(fz.h, e.data_ptr(), emap.shape[1], emap.shape[0], 1,
                                          small.data_ptr(), small.data_ptr(), 1, 1, 512,
                                          float(ZR[0]), float(ZR[1]), None, out.data_ptr())
    assert rc == panofuse.PF_EINVAL
    msg = fz.L.pf_last_error(fz.h).decode()
    assert "pf_merge_disparity_weighted" in msg and "2^30" in msg, msg
    gen = torch.Generator(device=DEV).manual_seed(5)
    tiles = torch.rand((1, fz.tile_elems), generator=gen, dtype=torch.float32, device=DEV)
    ones = torch.ones(fz.tile_elems, dtype=torch.float32, device=DEV)
    n = full.ntiles
    c64 = torch.zeros((1, n, 4), dtype=torch.float64, device=DEV)
    sm = torch.zeros((1, n, 6), dtype=torch.float64, device=DEV)
    fz.register_disparity_weighted(e, tiles, ones, ZR, apply=False, coeffs64=c64, summary=sm)
    p64 = torch.zeros((1, n, 4), dtype=torch.float64, device=DEV)
    psm = torch.zeros((1, n, 4), dtype=torch.float64, device=DEV)
    fz.register_disparity(e, tiles, ZR, apply=False, coeffs64=p64, summary=psm)
    fz.synchronize()
    got, want = c64.cpu().numpy(), p64.cpu().numpy()
    s6 = sm.cpu().numpy()
    del tiles, ones
    torch.cuda.empty_cache()
    assert _same(got, want) and np.isfinite(want).any()
    assert _same(s6[..., :4], psm.cpu().numpy())
    assert (s6[0, :, 4] >= 3).all() and np.array_equal(s6[0, :, 4], s6[0, :, 5])
    fz.close()


# ---- 9. isolation -------------------------------------------------------------------------------
def test_existing_calls_after_the_weighted_ones():
    """pf_merge_disparity, pf_merge and pf_merge_weighted on a context that ran the new calls give
    a fresh context's results (the golden file's for pf_merge) with a fresh context's launches."""
    g = np.load(GOLDEN)
    gtiles, gemap, gdata = WR.golden_inputs()
    lay, tiles, emap, disp = CS.c1(0)

    def run(fz):
        res = {}
        for name in ("merge_disparity", "merge", "merge_weighted"):
            em, data = (emap, disp) if name == "merge_disparity" else (gemap, gdata)
            out = torch.zeros((1, 256, 512), dtype=torch.int16, device=DEV)
            cf = torch.zeros((1, 6, 4), dtype=torch.float32, device=DEV)
            args = (_dev(em[None]), _dev(np.asarray(data)[None]))
            if name == "merge_weighted":
                args += (_dev(c1_tent()),)
            fz.profile(True)
            getattr(fz, name)(*args, out, ZR, coeffs=cf)
            fz.synchronize()
            launches = {k: v[2] for k, v in fz.profile_read().items()}
            fz.profile(False)
            res[name] = (out.cpu().numpy().view(np.uint16)[0], cf.cpu().numpy()[0], launches)
        return res

    fresh = run(_fuser(lay))
    used = _fuser(lay)
    _merge_w(used, emap, disp, CS.c1_field())
    _register_w(used, emap, disp, c1_tent(), apply=True)
    used.range_weights(_dev(disp[None]), 0.0, INF)
    after = run(used)
    for name in fresh:
        assert np.array_equal(after[name][0], fresh[name][0]), name
        assert np.array_equal(_bits(after[name][1]), _bits(fresh[name][1])), name
        assert after[name][2] == fresh[name][2], (name, after[name][2], fresh[name][2])
    assert np.array_equal(after["merge"][0], g["out_u16"])
    assert np.array_equal(_bits(after["merge"][1]), _bits(g["abcd"]))
    # the weighted disparity merge: one launch more than pf_merge_disparity's registration (the
    # sample weights), and the general Jacobi passes of a data-dependent coverage
    used.profile(True)
    _merge_w(used, emap, disp, np.ones(disp.size, f32))
    wl = {k: v[2] for k, v in used.profile_read().items()}
    used.profile(False)
    assert wl["register"] == fresh["merge_disparity"][2]["register"] + 1
    assert wl["jacobi"] == fresh["merge_weighted"][2]["jacobi"]
