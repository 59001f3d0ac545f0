"""GPU parity on the reference's other tile tables (midas, fold4, fold3) and the layout audit.

At a 512-wide output these tables -- and leres -- have stencil taps that leave their tile at the
coarse levels (tests/test_layouts.py pins the oracle's counts): the reference reads past the
buffer there, the oracle and k_tapmap clamp the linear index to [0, n - channels].  No earlier
GPU test ran where that count is non-zero, so the tap maps, the depth merge and the disparity
merge are held to the oracle here at exactly that size, bit for bit, and pf_layout_audit
(k_layout_audit) must count what the oracle counts.

Shapes: 512 x 256 output, 128 x 64 baseline, batch 2, tiles of 256 x 256 (fold3: 256 x 192, leres:
256 x 247); the audit also at 2048 with 64 x 64 tiles, where leres' and fold3's last levels leave
interior pixels uncovered."""
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
OUT_W, EW, BATCH = 512, 128, 2
MAKE = {"LERES": PL.leres_layout, "MIDAS": PL.midas_layout, "FOLD4": PL.fold4_layout,
        "FOLD3": PL.fold3_layout}
TILE = {"LERES": (256, 247), "MIDAS": (256, 256), "FOLD4": (256, 256), "FOLD3": (256, 192)}
NEW = ["MIDAS", "FOLD4", "FOLD3"]
# levels of the 512 output whose taps leave their tile (tests/test_layouts.py::TAPS_OUTSIDE)
OUTSIDE_LEVELS = {"LERES": (0,), "MIDAS": (0, 1), "FOLD4": (0, 1), "FOLD3": (0,)}


@pytest.fixture(scope="module")
def fuser():
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected on a host without a GPU")
    return panofuse.Fuser(0)


def _layout(cfg):
    return MAKE[cfg](*TILE[cfg])


_CASES = {}


def _case(cfg):
    """Inputs built as tests/test_gpu_parity.py::_inputs builds them (one seed per panorama) and
    the oracle's merge of each; computed once per layout and left unchanged."""
    if cfg in _CASES:
        return _CASES[cfg]
    lay = _layout(cfg)
    tiles, total = O.make_tiles(lay)
    emaps, datas, refs = [], [], []
    for seed in range(BATCH):
        seeds = pf_synth.seeds_for(1, 20261015 + 101 * seed)
        emap = pf_synth.baseline_emap(seeds, EW, EW // 2)[0].numpy()
        gt = pf_synth.scene_depth(seeds, OUT_W, OUT_W // 2)[0].numpy()
        resp = pf_synth.responses(seeds, lay.ntiles)
        data = O.warp_depth(gt, tiles, total, O.responses(resp))
        emaps.append(emap)
        datas.append(data)
        refs.append(O.merge(emap, tiles, data.copy(), OUT_W, ZR))
    _CASES[cfg] = {"lay": lay, "tiles": tiles, "total": total, "emaps": np.stack(emaps),
                   "datas": np.stack(datas), "refs": refs}
    return _CASES[cfg]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _band(out_w):
    lv = O.level_dims(out_w, out_w // 2, ZR, O.num_levels(out_w) - 1)
    return slice(lv.h0, lv.h1 + 1)


@pytest.mark.parametrize("cfg", NEW + ["LERES"])
def test_tap_index_maps_with_clamped_taps(fuser, cfg):
    lay = _layout(cfg)
    fuser.set_tiles(lay)
    tiles, total = O.make_tiles(lay)
    zeros = np.zeros(total, np.float32)
    clamped = 0
    for level in range(O.num_levels(OUT_W)):
        lv = O.level_dims(OUT_W, OUT_W // 2, ZR, level)
        got = fuser.probe_taps(OUT_W, ZR, level).cpu().numpy()
        ref = O.probe_taps(tiles, lv)
        assert got.shape == ref.shape
        bad = int((got != ref).sum())
        assert bad == 0, f"{cfg} level {level}: {bad} tap indices differ"
        _, _, oops, oob = O.targets(tiles, zeros, lv)
        assert (oops > 0) == (level in OUTSIDE_LEVELS[cfg])
        clamped += oob
    assert clamped > 0  # the ground this test is about


@pytest.mark.parametrize("cfg", NEW)
def test_merge_bit_exact(fuser, cfg):
    k = _case(cfg)
    lay = k["lay"]
    for ref, _ in k["refs"]:
        assert (ref[_band(OUT_W)] != 0).all(), "the oracle's own output must fill the band"
    fuser.set_tiles(lay)
    out = torch.zeros((BATCH, OUT_W // 2, OUT_W), dtype=torch.int16, device=DEV)
    coeffs = torch.zeros((BATCH, lay.ntiles, 4), dtype=torch.float32, device=DEV)
    t_tiles = _dev(k["datas"])
    fuser.merge(_dev(k["emaps"]), t_tiles, out, ZR, coeffs=coeffs)
    got = out.cpu().numpy().view(np.uint16)
    assert np.array_equal(t_tiles.cpu().numpy(), k["datas"]), "merge must not modify the tiles"
    for b, (ref, abcd) in enumerate(k["refs"]):
        assert np.array_equal(coeffs.cpu().numpy()[b], abcd), b
        assert np.array_equal(got[b], ref), f"pano {b}: {int((got[b] != ref).sum())} pixels differ"


def _to_disparity(data, tiles):
    """Per-tile normalised inverse depth, MiDaS' convention (tests/test_gpu_disp.py)."""
    out = np.empty_like(data)
    for t in tiles:
        n = t.width * t.height * t.channels
        inv = np.float32(1.0) / np.maximum(data[t.offset:t.offset + n], np.float32(0.02))
        lo, hi = inv.min(), inv.max()
        out[t.offset:t.offset + n] = (inv - lo) / (hi - lo)
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def test_merge_disparity_midas(fuser):
    """tests/test_gpu_disp.py::test_merge_disparity's comparison on the table the disparity
    registration exists for: coefficients equal to the restatement's (tests/disp_ref.py) bit for
    bit, and the panorama equal to the oracle's SolveDepthAll on the tiles the restatement
    transforms."""
    k = _case("MIDAS")
    lay, tiles = k["lay"], k["tiles"]
    disps = np.stack([_to_disparity(k["datas"][b], tiles) for b in range(BATCH)])
    fuser.set_tiles(lay)
    t_emap, t_tiles = _dev(k["emaps"]), _dev(disps)
    out = torch.zeros((BATCH, OUT_W // 2, OUT_W), dtype=torch.int16, device=DEV)
    cf = torch.zeros((BATCH, lay.ntiles, 4), dtype=torch.float32, device=DEV)
    fuser.merge_disparity(t_emap, t_tiles, out, ZR, coeffs=cf)
    fuser.synchronize()
    merged = out.cpu().numpy().view(np.uint16)
    assert np.array_equal(t_tiles.cpu().numpy(), disps)  # the caller's tiles stay
    for b in range(BATCH):
        xf = disps[b].copy()
        for p, t in enumerate(tiles):
            xs, ys, _, _ = O.reg_samples(t, disps[b], k["emaps"][b], ZR)
            r64, _ = R.fit(xs, ys)
            abcd = r64.astype(np.float32)
            assert np.array_equal(_bits(cf.cpu().numpy()[b, p]), _bits(abcd)), (b, p)
            n = t.width * t.height
            xf[t.offset:t.offset + n] = R.transform(disps[b][t.offset:t.offset + n], abcd)
        want, _ = O.solve_depth_all(k["emaps"][b], tiles, xf, OUT_W, ZR)
        assert (want[_band(OUT_W)] != 0).all()
        assert np.array_equal(merged[b], want), b


def _audit_reference(lay, out_w):
    tiles, total = O.make_tiles(lay)
    zeros = np.zeros(total, np.float32)
    ref = []
    for level in range(O.num_levels(out_w)):
        lv = O.level_dims(out_w, out_w // 2, ZR, level)
        _, n, oops, oob = O.targets(tiles, zeros, lv)
        ref.append({"w": lv.w, "h": lv.h, "h0": lv.h0, "h1": lv.h1, "taps_outside": oops,
                    "taps_clamped": oob, "covered": int((n > 0).sum()),
                    "uncovered_interior": int((n[lv.h0 + 1:lv.h1, 1:] == 0).sum()),
                    "max_cover": int(n.max()), "seam": int(n[:, lv.w - 1].any())})
    return ref


@pytest.mark.parametrize("cfg,out_w,tile", [("LERES", 512, None), ("MIDAS", 512, None),
                                            ("FOLD4", 512, None), ("FOLD3", 512, None),
                                            ("LERES", 2048, (64, 64)), ("FOLD3", 2048, (64, 64))])
def test_layout_audit_equals_the_oracle(fuser, cfg, out_w, tile):
    lay = MAKE[cfg](*(tile or TILE[cfg]))
    fuser.set_tiles(lay)
    ref = _audit_reference(lay, out_w)
    for level, want in enumerate(ref):
        got = fuser.layout_audit(out_w, ZR, level)
        print(f"{cfg} {out_w} level {level}: {got}")
        assert got == want, (cfg, out_w, level)
        assert fuser.layout_audit(out_w, ZR, level) == got  # the counters are zeroed per call
    if out_w == 512:
        assert [r["taps_outside"] > 0 for r in ref] == [lv in OUTSIDE_LEVELS[cfg] for lv in range(3)]
        assert ref[0]["taps_clamped"] > 0
    else:
        assert ref[-1]["uncovered_interior"] > 0 and ref[-1]["taps_outside"] == 0
    with pytest.raises(panofuse.PanofuseError):
        fuser.layout_audit(out_w, ZR, len(ref))


def test_layout_audit_follows_the_tile_size(fuser):
    """taps_outside is geometry; taps_clamped also depends on the tile size."""
    a = {}
    for size in ((256, 256), (64, 48)):
        lay = PL.midas_layout(*size)
        fuser.set_tiles(lay)
        a[size] = fuser.layout_audit(OUT_W, ZR, 0)
        assert a[size] == _audit_reference(lay, OUT_W)[0]
    assert a[(256, 256)]["taps_outside"] == a[(64, 48)]["taps_outside"] == 217
    assert a[(256, 256)]["covered"] == a[(64, 48)]["covered"]


@pytest.mark.parametrize("cfg", NEW)
def test_warp_rgb_bit_exact(fuser, cfg):
    """The RGB export's warp through each new table's windows: a 1000 x 500 panorama, tiles of a
    quarter of the export's size (256 wide, the export rule's height / 4)."""
    full = MAKE[cfg]()
    th = int(round(int(full.tile_h[0]) / 4))
    assert th == {"MIDAS": 182, "FOLD4": 247, "FOLD3": 187}[cfg]
    lay = MAKE[cfg](256, th)
    fuser.set_tiles(lay)
    tiles, _ = O.make_tiles(lay)
    rs = np.random.RandomState(11)
    h, w = 500, 1000
    yy, xx = np.mgrid[0:h, 0:w]
    pano = np.stack([(xx * 255 // (w - 1)), (yy * 255 // (h - 1)),
                     rs.randint(0, 256, size=(h, w))], -1).astype(np.uint8)
    ref = O.warp_rgb(pano, tiles)
    out = torch.zeros((1, ref.size), dtype=torch.uint8, device=DEV)
    fuser.warp_rgb(_dev(pano)[None], out)
    assert np.array_equal(out.cpu().numpy()[0], ref)
