"""The tile-pixel validity rule (pf_set_tile_validity) on the GPU, bit for bit against the CPU
compositions of tests/mask_ref.py (which tests/test_mask_ref.py proves against the oracle).

Shapes are C1 only: 6 tiles of 256^2, a 128x64 baseline, a 512x256 output.  The holes are a
rectangle of tile 0 (rows 100..255 x columns 100..179: it crosses the row two tiles share and
several 64x8 patch borders), a whole tile and a single pixel; written as NaN, or as 0.0 under
lo = 0.  The references are computed once per process (mask_ref's caches) and shared.  Other
output sizes, hole positions, layouts and channel counts: tests/test_gpu_mask_shapes.py.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import mask_ref as M  # noqa: E402
import panofuse  # noqa: E402
import pyoracle as O  # noqa: E402
from test_oracle import GOLDEN  # noqa: E402

ZR = M.ZR
DEV = "cuda:0"
W, H = M.OUT_W, M.OUT_H
INF = float("inf")


@pytest.fixture(scope="module")
def fuser():
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected on a host without a GPU")
    fz = panofuse.Fuser(0)
    fz.set_tiles(M.c1_inputs()[0])
    yield fz
    fz.set_tile_validity(None, None)


@pytest.fixture()
def masked(fuser):
    """The context with the rule "finite values only", switched off again afterwards."""
    fuser.set_tile_validity(-INF, INF)
    yield fuser
    fuser.set_tile_validity(None, None)


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a)).to(DEV)  # a copy: some inputs are read-only


def _same_bits(got, ref):
    """Equal bit for bit where ref is not NaN, NaN where it is."""
    got, ref = np.asarray(got), np.asarray(ref)
    nan = np.isnan(ref)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan], ref[~nan]))


def _fuse(fz, emap, data, coeffs=None):
    """fuse() of [B] panoramas: u16 [B][H][W]."""
    data = np.atleast_2d(data)
    B = data.shape[0]
    out = torch.zeros((B, H, W), dtype=torch.int16, device=DEV)
    e = _dev(np.broadcast_to(emap, (B,) + emap.shape))
    fz.fuse(e, _dev(data), out, ZR, coeffs=None if coeffs is None else _dev(coeffs))
    fz.synchronize()
    return out.cpu().numpy().view(np.uint16)


# ---- 1. registration ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def reg_case():
    """Two panoramas: the rectangle; the rectangle and an all-NaN tile.  With their references."""
    _, tiles, emap, data = M.c1_inputs()
    d = np.stack([M.with_holes(data, "rect"), M.with_holes(M.with_holes(data, "rect"), "tile")])
    ref = [M.register(tiles, d[b], emap) for b in range(2)]
    return tiles, emap, d, ref


def test_register_masked(masked, reg_case):
    tiles, emap, d, ref = reg_case
    e = _dev(np.stack([emap, emap]))
    t = _dev(d)
    c32 = torch.zeros((2, 6, 4), dtype=torch.float32, device=DEV)
    c64 = torch.zeros((2, 6, 4), dtype=torch.float64, device=DEV)
    masked.register(e, t, ZR, degree=3, apply=False, coeffs=c32, coeffs64=c64)
    counts = masked.tile_valid_counts(e, t, ZR)
    masked.synchronize()
    assert np.array_equal(t.cpu().numpy().view(np.uint32), d.view(np.uint32)), "apply=0 wrote"
    g64, g32, cn = c64.cpu().numpy(), c32.cpu().numpy(), counts.cpu().numpy()
    for b in range(2):
        r64, _, rcnt = ref[b]
        assert _same_bits(g64[b], r64), (b, g64[b], r64)
        assert _same_bits(g32[b], r64.astype(np.float32)), b
        assert np.array_equal(cn[b, :, 0], rcnt)
        assert np.array_equal(cn[b, :, 1], (~np.isnan(d[b].reshape(6, -1))).sum(1))
    assert np.isnan(g64[1, M.ALL_TILE]).all() and np.isnan(g32[1, M.ALL_TILE]).all()
    assert np.isfinite(g64[0]).all() and 0 < cn[0, 0, 0] < cn[0, 1, 0]


def test_register_masked_apply(masked, reg_case):
    tiles, emap, d, ref = reg_case
    t = _dev(d)
    c32 = torch.zeros((2, 6, 4), dtype=torch.float32, device=DEV)
    masked.register(_dev(np.stack([emap, emap])), t, ZR, degree=3, apply=True, coeffs=c32)
    masked.synchronize()
    got = t.cpu().numpy()
    for b in range(2):
        want = M.transform(tiles, d[b], ref[b][0].astype(np.float32))
        assert np.array_equal(np.isnan(got[b].reshape(6, -1)).sum(1)[:4],
                              np.isnan(d[b].reshape(6, -1)).sum(1)[:4])
        assert _same_bits(got[b], want), b
    assert np.isnan(got[1].reshape(6, -1)[M.ALL_TILE]).all()


def test_register_joint_masked(masked, reg_case):
    tiles, emap, d, ref = reg_case
    c64 = torch.zeros((2, 4), dtype=torch.float64, device=DEV)
    c32 = torch.zeros((2, 4), dtype=torch.float32, device=DEV)
    masked.register_joint(_dev(np.stack([emap, emap])), _dev(d), ZR, list(range(6)), coeffs=c32,
                          coeffs64=c64)
    masked.synchronize()
    for b in range(2):
        want = M.register_joint(ref[b][1], range(6))
        assert np.isfinite(want).all()
        assert _same_bits(c64.cpu().numpy()[b], want), b
        assert _same_bits(c32.cpu().numpy()[b], want.astype(np.float32)), b


# ---- 2. fusion, batch 1 ------------------------------------------------------------------------
@pytest.mark.parametrize("xform", [True, False], ids=["coeffs", "pretransformed"])
@pytest.mark.parametrize("hole", ["rect", "tile", "pixel"])
def test_fuse_masked_batch1(masked, hole, xform):
    _, tiles, emap, data = M.c1_inputs()
    abcd = M.c1_abcd()
    ref, stats = M.c1_masked(hole)
    if hole == "rect":  # the hole crosses a two-tile seam and leaves pixels un-windowed
        assert all(s["dropped"] > 0 and s["unwindowed"] > 0 for s in stats), stats
    raw = M.with_holes(data, hole)
    if xform:
        got = _fuse(masked, emap, raw, abcd[None])
    else:
        got = _fuse(masked, emap, M.transform(tiles, raw, abcd))
    diff = int((got[0] != ref).sum())
    assert diff == 0, f"{diff} pixels differ from the composition"


def test_fuse_check_and_merge_masked(masked):
    """pf_fuse_check (pf_fuse_targets + pf_fuse_level per level) and pf_merge (the masked
    registration, then the fusion; the all-NaN tile drops out through its NaN coefficients)."""
    _, tiles, emap, data = M.c1_inputs()
    ref, _ = M.c1_masked("rect")
    out = torch.zeros((1, H, W), dtype=torch.int16, device=DEV)
    err = masked.fuse_check(_dev(emap[None]), _dev(M.with_holes(data, "rect")[None]), ZR, W,
                            coeffs=_dev(M.c1_abcd()[None]), out=out)
    masked.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint16)[0], ref)
    assert np.isfinite(err.cpu().numpy()).all()

    d = M.with_holes(M.with_holes(data, "rect"), "tile")
    c64, _, _ = M.register(tiles, d, emap)
    want, _ = M.masked_fuse(emap, tiles, M.transform(tiles, d, c64.astype(np.float32)))
    cf = torch.zeros((1, 6, 4), dtype=torch.float32, device=DEV)
    masked.merge(_dev(emap[None]), _dev(d[None]), out, ZR, coeffs=cf)
    masked.synchronize()
    assert _same_bits(cf.cpu().numpy()[0], c64.astype(np.float32))
    assert np.array_equal(out.cpu().numpy().view(np.uint16)[0], want)


# ---- 3. fusion, batch 9 ------------------------------------------------------------------------
def test_fuse_masked_batch9(masked):
    """Two groups of panoramas per block, the second partly filled; every panorama has its own
    mask and panorama 3 has none: the counts are per panorama."""
    _, tiles, emap, data = M.c1_inputs()
    abcd = M.c1_abcd()
    d = np.stack([np.array(data) for _ in range(9)]).reshape(9, 6, 256, 256)
    d[1, 1, 100:160, :] = np.nan
    d[2, 2, :, 200:256] = np.nan
    d[4, 3, 60:200, 30:90] = np.nan
    d[5, 5, 128:, 128:] = np.nan
    d[6, 0, 0:128, 0:128] = np.nan
    d[6, 3, 250:256, :] = np.nan
    d = d.reshape(9, -1)
    d[0], d[7], d[8] = (M.with_holes(data, n) for n in ("rect", "tile", "pixel"))
    cf = np.broadcast_to(abcd, (9, 6, 4))
    got = _fuse(masked, emap, d, cf)
    for b, name in ((0, "rect"), (7, "tile"), (8, "pixel")):
        assert np.array_equal(got[b], M.c1_masked(name)[0]), name
    assert np.array_equal(got[3], M.c1_masked("none")[0])
    for b in (1, 2, 4, 5, 6):
        alone = _fuse(masked, emap, d[b], abcd[None])[0]
        assert np.array_equal(got[b], alone), b
        assert not np.array_equal(got[b], got[3]), b


# ---- 4. range mode -----------------------------------------------------------------------------
def test_range_mode(fuser):
    _, tiles, emap, data = M.c1_inputs()
    assert (data > 0).all(), "the case needs tiles without a zero of their own"
    try:
        fuser.set_tile_validity(lo=0.0)
        got = _fuse(fuser, emap, M.with_holes(data, "rect", 0.0), M.c1_abcd()[None])[0]
        assert np.array_equal(got, M.c1_masked("rect")[0])
        # a value equal to lo or to hi is invalid
        lo, hi = np.float32(0.25), np.float32(0.75)
        d = np.array(data).reshape(6, -1)
        d[0, :1000] = lo
        d[1, :2000] = hi
        d[2, :10] = np.nextafter(lo, np.float32(1))
        d[2, 10:20] = np.nextafter(hi, np.float32(0))
        fuser.set_tile_validity(float(lo), float(hi))
        cn = fuser.tile_valid_counts(_dev(emap[None]), _dev(d.reshape(1, -1)), ZR)
        fuser.synchronize()
        want = ((d > lo) & (d < hi)).sum(1)
        assert np.array_equal(cn.cpu().numpy()[0, :, 1], want)
        assert want[0] == ((d[0, 1000:] > lo) & (d[0, 1000:] < hi)).sum() and want[2] >= 20
    finally:
        fuser.set_tile_validity(None, None)
    with pytest.raises(panofuse.PanofuseError) as e:
        fuser.set_tile_validity(1.0, 1.0)
    assert e.value.code == panofuse.PF_EINVAL


# ---- 5. stitch ---------------------------------------------------------------------------------
@pytest.mark.parametrize("with_coeffs", [False, True], ids=["plain", "coeffs"])
def test_stitch_masked(masked, with_coeffs):
    _, tiles, emap, data = M.c1_inputs()
    abcd = M.c1_abcd()
    d = np.stack([M.with_holes(M.with_holes(data, "rect"), "tile"), M.with_holes(data, "pixel")])
    out = torch.full((2, H, W), -1, dtype=torch.int16, device=DEV)
    cf = _dev(np.broadcast_to(abcd, (2, 6, 4))) if with_coeffs else None
    masked.stitch(_dev(d), out, coeffs=cf)
    masked.synchronize()
    got = out.cpu().numpy().view(np.uint16)
    for b in range(2):
        want = M.stitch_valid(tiles, d[b], W, H, abcd if with_coeffs else None)
        assert np.array_equal(got[b], want), b
    plain = M.stitch_valid(tiles, data, W, H, abcd if with_coeffs else None)
    assert not np.array_equal(got[0], plain)


# ---- 6. default mode ---------------------------------------------------------------------------
def test_default_mode_is_unchanged(fuser):
    """After the rule was on and is off again: the golden bits and the launch counts of a context
    that never set it."""
    g = np.load(GOLDEN)
    emap = (g["emap_u16"].astype(np.float32) / np.float32(65535.0)).astype(np.float32)
    data = (g["tiles_u8"].astype(np.float32) / np.float32(255.0)).astype(np.float32)

    def run(fz):
        out = torch.zeros((1, H, W), dtype=torch.int16, device=DEV)
        cf = torch.zeros((1, 6, 4), dtype=torch.float32, device=DEV)
        fz.profile(True)
        fz.merge(_dev(emap[None]), _dev(data.reshape(1, -1)), out, ZR, coeffs=cf)
        fz.synchronize()
        prof = fz.profile_read()
        fz.profile(False)
        return out.cpu().numpy().view(np.uint16)[0], cf.cpu().numpy()[0], prof

    fuser.set_tile_validity(-INF, INF)
    on = run(fuser)
    fuser.set_tile_validity(None, None)
    got = run(fuser)
    fresh = panofuse.Fuser(0)
    fresh.set_tiles(M.c1_inputs()[0])
    ref = run(fresh)
    fresh.close()
    assert np.array_equal(got[0], g["out_u16"]) and np.array_equal(got[1], g["abcd"])
    assert np.array_equal(ref[0], g["out_u16"])
    assert {k: v[2] for k, v in got[2].items()} == {k: v[2] for k, v in ref[2].items()}
    # the rule on and nothing invalid: the same panorama through the marker-reading passes
    assert np.array_equal(on[0], g["out_u16"]) and np.array_equal(on[1], g["abcd"])


# ---- 7. entry points that cannot honour the rule -----------------------------------------------
def test_unsupported_entry_points(masked):
    _, tiles, emap, data = M.c1_inputs()
    e, t = _dev(emap[None]), _dev(np.array(data)[None])
    out = torch.zeros((1, H, W), dtype=torch.int16, device=DEV)
    lv = O.level_dims(W, H, ZR, 2)
    a = torch.zeros((lv.h, lv.w), dtype=torch.float32, device=DEV)
    b = torch.zeros((lv.h, lv.w), dtype=torch.float32, device=DEV)
    calls = {
        "pf_register_disparity": lambda: masked.register_disparity(e, t, ZR, apply=False),
        "pf_merge_disparity": lambda: masked.merge_disparity(e, t, out, ZR),
        "pf_solve_smoothing": lambda: masked.solve_smoothing(t, out, ZR),
        "pf_fuse_partial": lambda: masked.fuse_partial(t, None, 0, 6, W, ZR, 2, a, b),
        "pf_fuse_partial_rows": lambda: masked.fuse_partial_rows(t, None, 0, 6, W, ZR, 2,
                                                                 lv.h0, lv.h1, a, b),
        "pf_fuse_coverage_rows": lambda: masked.fuse_coverage_rows(W, ZR, 2, lv.h0, lv.h1, a),
        "pf_fuse_multicover": lambda: masked.multicover_count(W, ZR, 2),
        "pf_fuse_multicover_patch": lambda: masked.multicover_patch(W, ZR, 2, a, b),
    }
    for name, call in calls.items():
        with pytest.raises(panofuse.PanofuseError) as err:
            call()
        assert err.value.code == panofuse.PF_ESTATE, name
        assert "pf_set_tile_validity" in str(err.value) and name in str(err.value), name
    masked.set_tile_validity(None, None)
    for name, call in calls.items():  # and with the rule off they run
        call()
    masked.synchronize()
