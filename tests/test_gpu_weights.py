"""Per-pixel tile weights (pf_register_weighted, pf_fuse_weighted, pf_merge_weighted,
pf_tile_tent_weights) on the GPU, bit for bit against tests/weight_ref.py (which
tests/test_weight_ref.py proves against the oracle and tests/mask_ref.py).

Shapes: C1 (6 tiles of 256^2, 512x256), two output sizes of test_fuse_shapes.SHAPES (500x248, whose
level 0 takes the per-sweep Jacobi, and 440x220, whose level 0 has no coverage certificate) and the
small-tile layouts of tests/mask_shapes.py (LeReS 64x48, MiDaS 40x30, mixed off-grid sizes, three
channels), where out-of-tile taps are clamped and the weight index must follow the value index.
The weight fields are the tent and a fixed-seed smooth field (8x8 per tile, upsampled) with an
exact-zero rectangle.  Every reference is computed once per process and shared.
"""
import functools
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import mask_ref as M  # noqa: E402
import mask_shapes as MS  # noqa: E402
import panofuse  # noqa: E402
import weight_ref as WR  # noqa: E402
from test_oracle import GOLDEN  # noqa: E402

f32 = np.float32
ZR = M.ZR
DEV = "cuda:0"
INF = float("inf")


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a)).to(DEV)  # a copy: some inputs are read-only


def _same_bits(got, ref):
    """Equal bit for bit where ref is not NaN, NaN where it is."""
    got, ref = np.asarray(got), np.asarray(ref)
    nan = np.isnan(ref)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan], ref[~nan]))


def _fuser(lay, channels=1):
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected on a host without a GPU")
    fz = panofuse.Fuser(0)
    fz.set_tiles(lay, channels)
    return fz


@pytest.fixture(scope="module")
def fuser():
    return _fuser(M.c1_inputs()[0])


def _emaps(emap, B):
    return _dev(np.broadcast_to(emap, (B,) + np.shape(emap)))


def _merge_w(fz, emap, data, w, out_w=M.OUT_W):
    """merge_weighted of [B] panoramas: (u16 [B][H][W], coeffs float32 [B][n][4])."""
    data = np.atleast_2d(data)
    B = data.shape[0]
    out = torch.zeros((B, out_w // 2, out_w), dtype=torch.int16, device=DEV)
    cf = torch.zeros((B, fz.layout.ntiles, 4), dtype=torch.float32, device=DEV)
    fz.merge_weighted(_emaps(emap, B), _dev(data), _dev(w), out, ZR, coeffs=cf)
    fz.synchronize()
    return out.cpu().numpy().view(np.uint16), cf.cpu().numpy()


def _fuse_w(fz, emap, data, w, coeffs=None, out_w=M.OUT_W, out_h=M.OUT_H):
    data = np.atleast_2d(data)
    B = data.shape[0]
    out = torch.zeros((B, out_h, out_w), dtype=torch.int16, device=DEV)
    fz.fuse_weighted(_emaps(emap, B), _dev(data), _dev(w), out, ZR,
                     coeffs=None if coeffs is None else _dev(coeffs))
    fz.synchronize()
    return out.cpu().numpy().view(np.uint16)


def _register_w(fz, emap, data, w, apply=False):
    """(coeffs32 [B][n][4], coeffs64, summary [B][n][2], tiles after the call)."""
    data = np.atleast_2d(data)
    B, n = data.shape[0], fz.layout.ntiles
    t = _dev(data)
    c32 = torch.zeros((B, n, 4), dtype=torch.float32, device=DEV)
    c64 = torch.zeros((B, n, 4), dtype=torch.float64, device=DEV)
    sm = torch.zeros((B, n, 2), dtype=torch.float64, device=DEV)
    fz.register_weighted(_emaps(emap, B), t, _dev(w), ZR, apply=apply, coeffs=c32, coeffs64=c64,
                         summary=sm)
    fz.synchronize()
    return c32.cpu().numpy(), c64.cpu().numpy(), sm.cpu().numpy(), t.cpu().numpy()


def _merge_plain(fz, emap, data, out_w=M.OUT_W):
    data = np.atleast_2d(data)
    B = data.shape[0]
    out = torch.zeros((B, out_w // 2, out_w), dtype=torch.int16, device=DEV)
    cf = torch.zeros((B, fz.layout.ntiles, 4), dtype=torch.float32, device=DEV)
    fz.merge(_emaps(emap, B), _dev(data), out, ZR, coeffs=cf)
    fz.synchronize()
    return out.cpu().numpy().view(np.uint16), cf.cpu().numpy()


# ---- the weight fields --------------------------------------------------------------------------
def smooth_field(tiles, seed, junk=True):
    """A fixed-seed weight set: per tile an 8 x 8 grid of values in [0.1, 1] upsampled bilinearly
    to the tile, in channel 0; the other channels hold non-zero junk."""
    rs = np.random.RandomState(seed)
    total = sum(t.width * t.height * t.channels for t in tiles)
    out = (rs.rand(total).astype(f32) * f32(3) - f32(1.5)) if junk else np.zeros(total, f32)
    for t in tiles:
        w, h, c = t.width, t.height, t.channels
        g = (0.1 + 0.9 * rs.rand(8, 8)).astype(np.float64)
        ys = np.linspace(0, 7, h)
        xs = np.linspace(0, 7, w)
        y0 = np.minimum(ys.astype(int), 6)
        x0 = np.minimum(xs.astype(int), 6)
        fy = (ys - y0)[:, None]
        fx = (xs - x0)[None, :]
        v = ((1 - fy) * (1 - fx) * g[y0][:, x0] + (1 - fy) * fx * g[y0][:, x0 + 1]
             + fy * (1 - fx) * g[y0 + 1][:, x0] + fy * fx * g[y0 + 1][:, x0 + 1])
        out[t.offset:t.offset + w * h * c:c] = v.astype(f32).reshape(-1)
    return out


def zero_rect(tiles, weights, p=0):
    """`weights` with an exact-zero rectangle in tile p: rows 39 % .. 100 % and columns 39 % .. 70 %
    of the tile (at C1 this is mask_ref.RECT: it crosses the row two tiles share and several
    64-column patch borders)."""
    w = np.array(weights, f32)
    t = tiles[p]
    v = w[t.offset:t.offset + t.width * t.height * t.channels].reshape(t.height, t.width,
                                                                       t.channels)
    v[int(t.height * 100 / 256):, int(t.width * 100 / 256):int(t.width * 180 / 256), 0] = 0.0
    return w


@functools.lru_cache(maxsize=None)
def c1_field():
    _, tiles, _, _ = M.c1_inputs()
    w = zero_rect(tiles, smooth_field(tiles, 20261021))
    assert not w.reshape(6, 256, 256)[M.RECT].any()
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def c1_tent():
    w = WR.tent(M.c1_inputs()[1])
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def c1_merge_ref(kind):
    _, tiles, emap, data = M.c1_inputs()
    return WR.merge(emap, tiles, data, {"tent": c1_tent, "field": c1_field}[kind]())


# ---- 1. ones ------------------------------------------------------------------------------------
def test_ones_is_the_plain_merge(fuser):
    g = np.load(GOLDEN)
    tiles, emap, data = WR.golden_inputs()
    ones = np.ones(data.size, f32)
    out, cf = _merge_w(fuser, emap, data, ones)
    assert np.array_equal(cf[0].view(np.uint32), g["abcd"].view(np.uint32))
    assert np.array_equal(out[0], g["out_u16"])
    pout, pcf = _merge_plain(fuser, emap, data)
    assert np.array_equal(out, pout) and np.array_equal(cf.view(np.uint32), pcf.view(np.uint32))
    # register_weighted alone; apply transforms the tiles as pf_register's does
    c32, c64, sm, after = _register_w(fuser, emap, data, ones, apply=True)
    assert np.array_equal(c32[0].view(np.uint32), g["abcd"].view(np.uint32))
    assert np.array_equal(c64[0].astype(f32).view(np.uint32), g["abcd"].view(np.uint32))
    assert np.array_equal(sm[0, :, 0], sm[0, :, 1]) and (sm[0, :, 0] > 4).all()
    assert np.array_equal(after[0], M.transform(tiles, data, g["abcd"]))
    # fuse_weighted with the coefficients, and on the transformed tiles without
    assert np.array_equal(_fuse_w(fuser, emap, data, ones, g["abcd"][None])[0], g["out_u16"])
    assert np.array_equal(_fuse_w(fuser, emap, after[0], ones)[0], g["out_u16"])


# ---- 2. weights in {0, 1} are the validity rule ---------------------------------------------------
@pytest.fixture(scope="module")
def masked_ctx():
    fz = _fuser(M.c1_inputs()[0])
    fz.set_tile_validity(-INF, INF)
    return fz


@pytest.mark.parametrize("name", ["rect", "tile", "pixel"])
def test_zero_one_weights_are_the_validity_rule(fuser, masked_ctx, name):
    _, tiles, emap, data = M.c1_inputs()
    holed = M.with_holes(data, name)
    w = M.with_holes(np.ones(data.size, f32), name, value=0.0)
    # mask_ref: its registration, then its masked fusion under those coefficients
    r64, _, rcnt = M.register(tiles, holed, emap)
    ref, _ = M.masked_fuse(emap, tiles, M.transform(tiles, holed, r64.astype(f32)))
    out, cf = _merge_w(fuser, emap, holed, w)
    assert _same_bits(cf[0], r64.astype(f32))
    assert np.array_equal(out[0], ref)
    _, _, sm, _ = _register_w(fuser, emap, holed, w)
    assert np.array_equal(sm[0, :, 0], rcnt) and np.array_equal(sm[0, :, 1], rcnt)
    # the library's own run under the rule
    mout, mcf = _merge_plain(masked_ctx, emap, holed)
    assert np.array_equal(out, mout) and _same_bits(cf, mcf)
    # fuse_weighted under the unmasked coefficients: mask_ref's cached case
    got = _fuse_w(fuser, emap, holed, w, M.c1_abcd()[None])
    assert np.array_equal(got[0], M.c1_masked(name)[0])


# ---- 3. tent and a smooth field -----------------------------------------------------------------
@pytest.mark.parametrize("kind", ["tent", "field"])
def test_c1_weighted_merge(fuser, kind):
    _, tiles, emap, data = M.c1_inputs()
    w = {"tent": c1_tent, "field": c1_field}[kind]()
    ref, rabcd = c1_merge_ref(kind)
    out, cf = _merge_w(fuser, emap, data, w)
    assert np.array_equal(cf[0].view(np.uint32), rabcd.view(np.uint32))
    assert np.array_equal(out[0], ref)
    plain, _ = _merge_plain(fuser, emap, data)
    assert (out != plain).any(), "the weights must matter"


def test_per_level_gather_is_the_one_launch_gather(fuser):
    """PF_WTGT_LEVELS=1: one k_targets_patch_weighted launch per level."""
    _, tiles, emap, data = M.c1_inputs()
    ref, _ = c1_merge_ref("field")
    os.environ["PF_WTGT_LEVELS"] = "1"
    try:
        fuser.profile(True)
        out, _ = _merge_w(fuser, emap, data, c1_field())
        launches = fuser.profile_read()["targets"][2]
    finally:
        del os.environ["PF_WTGT_LEVELS"]
        fuser.profile(False)
    assert launches == 3
    assert np.array_equal(out[0], ref)


def _case_check(case, fz, w):
    """register_weighted + fuse_weighted of one mask_shapes case against weight_ref."""
    r64, rsum, _ = WR.register(case.tiles, case.data, w, case.emap)
    rabcd = r64.astype(f32)
    ref = WR.fuse(case.emap, case.tiles, case.data, w, rabcd, case.out_w, case.out_h)
    c32, c64, sm, _ = _register_w(fz, case.emap, case.data, w)
    assert _same_bits(c64[0], r64) and _same_bits(c32[0], rabcd)
    assert np.array_equal(sm[0].view(np.uint64), rsum.view(np.uint64))
    got = _fuse_w(fz, case.emap, case.data, w, c32, case.out_w, case.out_h)
    assert np.array_equal(got[0], ref)
    return got[0], c32


@pytest.mark.parametrize("size", [(500, 248), (440, 220)], ids=MS.size_id)
@pytest.mark.parametrize("kind", ["tent", "field"])
def test_output_sizes(size, kind):
    case = MS.row_case(size)
    w = c1_tent() if kind == "tent" else c1_field()
    _case_check(case, _fuser(case.lay), w)


# ---- 4. the weight index follows the value index ------------------------------------------------
@pytest.mark.parametrize("name", MS.LAYOUTS)
def test_tile_shapes(name):
    case = MS.layout_case(name)
    if name in ("LERES", "MIDAS"):  # the clamped-tap cases
        assert any(m[2].any() for m in MS.tile_maps(case, 0))
    w = zero_rect(case.tiles, smooth_field(case.tiles, 7 + len(name)))
    fz = _fuser(case.lay, case.channels)
    got, c32 = _case_check(case, fz, w)
    if case.channels == 3:  # the junk of channels 1-2 does not matter
        w0 = np.array(w)
        w0[1::3] = 0.0
        w0[2::3] = 0.0
        assert (w0 != w).any()
        again = _fuse_w(fz, case.emap, case.data, w0, c32, case.out_w, case.out_h)
        assert np.array_equal(again[0], got)


# ---- 5. batches ---------------------------------------------------------------------------------
def test_batch_of_three(fuser):
    _, tiles, emap, data = M.c1_inputs()
    ones = np.ones(data.size, f32)
    w = np.stack([ones, M.with_holes(ones, "tile", value=0.0), c1_field()])
    d = np.stack([data, data, data])
    out, cf = _merge_w(fuser, emap, d, w)
    for b in range(3):
        o1, c1 = _merge_w(fuser, emap, data, w[b])
        assert np.array_equal(out[b], o1[0]) and _same_bits(cf[b], c1[0]), b
    assert np.array_equal(out[2], c1_merge_ref("field")[0])
    assert np.isnan(cf[1, M.ALL_TILE]).all() and np.isfinite(cf[0]).all()
    # one shared set is three copies of it
    tent = c1_tent()
    shared, scf = _merge_w(fuser, emap, d, tent)
    copies, ccf = _merge_w(fuser, emap, d, np.stack([tent] * 3))
    assert np.array_equal(shared, copies) and np.array_equal(scf, ccf)
    assert np.array_equal(shared[1], c1_merge_ref("tent")[0])


def test_batch_across_panorama_groups(fuser):
    """Batch 6 with per-panorama weights: two groups of four panoramas per wave, the second
    half full."""
    _, tiles, emap, data = M.c1_inputs()
    ones = np.ones(data.size, f32)
    sets = [c1_field(), ones, c1_tent(), M.with_holes(ones, "rect", value=0.0), c1_tent(),
            c1_field()]
    out, _ = _merge_w(fuser, emap, np.stack([data] * 6), np.stack(sets))
    assert np.array_equal(out[0], c1_merge_ref("field")[0])
    assert np.array_equal(out[5], c1_merge_ref("field")[0])
    assert np.array_equal(out[2], c1_merge_ref("tent")[0])
    assert np.array_equal(out[4], c1_merge_ref("tent")[0])
    assert np.array_equal(out[1], _merge_plain(fuser, emap, data)[0][0])
    assert np.array_equal(out[3], _merge_w(fuser, emap, data, sets[3])[0][0])


# ---- 6. registration edge cases -----------------------------------------------------------------
def test_registration_edge_cases(fuser):
    """Tile 0 keeps exactly 3 samples, tile 1 exactly 4, tile 2 none; tile 3 has odd weights
    (NaN, negative, +inf: unusable; a denormal and a huge one: usable)."""
    _, tiles, emap, data = M.c1_inputs()
    w = np.array(c1_field())

    def keep(p, k):
        el = WR.sample_elements(tiles[p], emap)
        vals, counts = np.unique(el, return_counts=True)
        once = vals[counts == 1]
        chosen = once[np.linspace(0, once.size - 1, k).astype(int)]
        assert np.unique(chosen).size == k
        t = tiles[p]
        kept = w[t.offset + chosen].copy()
        assert (kept > 0).all()
        w[t.offset:t.offset + t.width * t.height] = 0.0
        w[t.offset + chosen] = kept

    keep(0, 3)
    keep(1, 4)
    w[tiles[2].offset:tiles[2].offset + 65536] = 0.0
    el3 = np.unique(WR.sample_elements(tiles[3], emap))
    odd = np.array([np.nan, -1.0, np.inf, -0.0, 1e-40, 3e38], f32)
    w[tiles[3].offset + el3[:odd.size]] = odd
    r64, rsum, _ = WR.register(tiles, data, w, emap)
    assert list(rsum[:3, 0]) == [3, 4, 0]
    assert np.isnan(r64[0]).all() and np.isfinite(r64[1]).all() and np.isnan(r64[2]).all()
    c32, c64, sm, after = _register_w(fuser, emap, data, w)
    assert np.array_equal(after[0].view(np.uint32), np.asarray(data).view(np.uint32))
    assert np.array_equal(sm[0].view(np.uint64), rsum.view(np.uint64))  # counts and sum of w
    assert _same_bits(c64[0], r64) and _same_bits(c32[0], r64.astype(f32))


# ---- 7. the tent --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["C1", "MIXED", "LERES3"])
def test_tent_weights(fuser, name):
    if name == "C1":
        fz, tiles = fuser, M.c1_inputs()[1]
    else:
        case = MS.layout_case(name)
        fz, tiles = _fuser(case.lay, case.channels), case.tiles
    out = torch.full((fz.tile_elems,), -3.0, dtype=torch.float32, device=DEV)
    got = fz.tent_weights(out)
    fz.synchronize()
    ref = WR.tent(tiles)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), ref.view(np.uint32))
    assert ref[::tiles[0].channels].min() > 0 and ref.max() == 1.0


# ---- 8. refusals --------------------------------------------------------------------------------
def _calls(fz, emap, data, w):
    B = 1
    e, t, wt = _emaps(emap, B), _dev(data[None]), _dev(w)
    out = torch.zeros((B, M.OUT_H, M.OUT_W), dtype=torch.int16, device=DEV)
    return {"pf_tile_tent_weights": lambda: fz.tent_weights(),
            "pf_register_weighted": lambda: fz.register_weighted(e, t, wt, ZR, apply=False),
            "pf_fuse_weighted": lambda: fz.fuse_weighted(e, t, wt, out, ZR),
            "pf_merge_weighted": lambda: fz.merge_weighted(e, t, wt, out, ZR)}


def test_refusals():
    _, tiles, emap, data = M.c1_inputs()
    fz = _fuser(M.c1_inputs()[0])
    calls = _calls(fz, emap, np.asarray(data), c1_tent())
    modes = [("pf_set_tile_validity", lambda: fz.set_tile_validity(-INF, INF),
              lambda: fz.set_tile_validity(None, None)),
             ("pf_set_register_loss", lambda: fz.set_register_loss("huber", 0.1),
              lambda: fz.set_register_loss(None)),
             ("pf_set_tile_depth", lambda: fz.set_tile_depth("planar"),
              lambda: fz.set_tile_depth("ray"))]
    for setter, on, off in modes:
        on()
        try:
            for entry, call in calls.items():
                with pytest.raises(panofuse.PanofuseError) as err:
                    call()
                assert err.value.code == panofuse.PF_ESTATE, (setter, entry)
                assert setter in str(err.value) and entry in str(err.value), str(err.value)
        finally:
            off()
        for call in calls.values():  # and they run again
            call()
        fz.synchronize()
    e, t = _emaps(emap, 3), _dev(np.stack([data] * 3))
    out = torch.zeros((3, M.OUT_H, M.OUT_W), dtype=torch.int16, device=DEV)
    two = _dev(np.stack([c1_tent()] * 2))
    for call in (lambda: fz.merge_weighted(e, t, None, out, ZR),
                 lambda: fz.register_weighted(e, t, None, ZR),
                 lambda: fz.fuse_weighted(e, t, None, out, ZR),
                 lambda: fz.merge_weighted(e, t, two, out, ZR),
                 lambda: fz.register_weighted(e, t, two, ZR),
                 lambda: fz.fuse_weighted(e, t, two, out, ZR)):
        with pytest.raises(panofuse.PanofuseError) as err:
            call()
        assert err.value.code == panofuse.PF_EINVAL, str(err.value)
    fz.set_solver("normal")
    try:
        for name in ("pf_register_weighted", "pf_merge_weighted"):
            with pytest.raises(panofuse.PanofuseError) as err:
                calls[name]()
            assert err.value.code == panofuse.PF_EINVAL and "pf_set_solver" in str(err.value)
    finally:
        fz.set_solver("lm")
    with pytest.raises(ValueError):
        fz.merge_weighted(e, t, _dev(np.ones(5, f32)), out, ZR)


# ---- 9. isolation -------------------------------------------------------------------------------
def test_plain_merge_after_a_weighted_one():
    g = np.load(GOLDEN)
    tiles, emap, data = WR.golden_inputs()

    def plain(fz):
        fz.profile(True)
        out, cf = _merge_plain(fz, emap, data)
        stages = fz.profile_read()
        fz.profile(False)
        return out, cf, {k: v[2] for k, v in stages.items()}

    fresh = _fuser(M.c1_inputs()[0])
    fout, fcf, flaunches = plain(fresh)
    used = _fuser(M.c1_inputs()[0])
    _merge_w(used, emap, data, c1_field())
    uout, ucf, ulaunches = plain(used)
    assert np.array_equal(uout[0], g["out_u16"]) and np.array_equal(ucf[0], g["abcd"])
    assert np.array_equal(uout, fout) and np.array_equal(ucf, fcf)
    assert ulaunches == flaunches, (ulaunches, flaunches)
    # a weighted merge takes the general Jacobi passes: its launch counts are those of a merge
    # under the validity rule
    fresh.set_tile_validity(-INF, INF)
    _, _, mlaunches = plain(fresh)
    used.profile(True)
    _merge_w(used, emap, data, np.ones(data.size, f32))
    wlaunches = {k: v[2] for k, v in used.profile_read().items()}
    used.profile(False)
    assert wlaunches == mlaunches, (wlaunches, mlaunches)
