"""GPU parity on tile shapes pf_set_tiles accepts and no other GPU test runs (tests/tile_shapes.py
has the cases, tests/test_tile_shapes.py checks them and the oracle on the CPU):

* tile sizes that are not whole 64 x 32 patches, in one layout of six different sizes: lanes of
  k_warp_depth outside their tile (patch_pixel == 0, the dropped store through the out-of-range
  buffer offset, the cut patches of warp_patches_host / k_patch_box / k_warp_local) on each of
  the eight staging paths, and g.off / g.pix_off where the tiles differ;
* the smallest tiles (2 x 2 up);
* the staged RGB warp with partial patch columns, and its fall-back when a width is no multiple
  of 4;
* tiles of 3 interleaved channels through every entry point that takes tiles;
* the mixed layout through the fusion.

Every comparison is bit for bit, against the oracle and -- for the depth warp without a response
-- against a numpy gather that shares no code with it.  Outputs of the warps sit between guard
words that must keep their sentinel.
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
import stitch_ref as S  # noqa: E402
import tile_shapes as TS  # noqa: E402

ZR = PL.ZENITH_RANGE
DEV = "cuda:0"
GUARD = 64  # guard elements before the first and after the last panorama's tile block
SENTINEL = -12345.0  # no warp output: depths and responses are in [0, 1]
B_WARP = 17  # one full 16-panorama chunk of the warps + a ragged one
CHECKED = (0, 15, 16)
OUT_W, EW, BATCH = TS.OUT_W, TS.EW, TS.BATCH


@pytest.fixture(scope="module")
def fuser():
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected on a host without a GPU")
    f = panofuse.Fuser(0)
    yield f
    f.close()


@pytest.fixture(scope="module")
def fuser3(fuser):
    """A second context, for the layout under comparison (3 channels, or one tile alone)."""
    f = panofuse.Fuser(0)
    yield f
    f.close()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Guarded:
    """A packed [B, n] device tensor (the binding takes contiguous tensors and the kernels stride
    by n) cut out of a buffer with GUARD sentinel elements on either side."""

    def __init__(self, B, n, dtype=torch.float32, fill=SENTINEL):
        self.flat = torch.full((GUARD + B * n + GUARD,), fill, dtype=dtype, device=DEV)
        self.t = self.flat[GUARD:GUARD + B * n].view(B, n)
        self.fill = fill
        assert self.t.is_contiguous()

    def host(self):
        """The [B, n] result; asserts that both guards still hold the sentinel."""
        torch.cuda.synchronize()
        h = self.flat.cpu().numpy()
        assert (h[:GUARD] == self.fill).all(), "written before the first panorama's tiles"
        assert (h[-GUARD:] == self.fill).all(), "written past the last panorama's tiles"
        return h[GUARD:-GUARD].reshape(self.t.shape)


def _panoramas(pw, ph, B, base):
    """B distinct float32 panoramas from three scenes (scene b % 3 scaled by 1 - b/64)."""
    scenes = pf_synth.scene_depth(pf_synth.seeds_for(3, base), pw, ph).numpy()
    return np.stack([scenes[b % 3] * np.float32(1.0 - b / 64.0) for b in range(B)])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


# ------------------------------------------------------------------------------------------
# 1. the depth warp, off-grid and mixed
def test_warp_depth_mixed_sizes_every_path(fuser, fuser3):
    """The mixed layout on one context at the five panorama sizes in turn (the cached map follows
    the size), batch 17, with per-panorama responses and without.  The case table gives every
    staging path a patch cut in X and one cut in Y -- asserted here, from the same list the run
    uses.  Each tile alone, as a one-tile layout, must equal its slice of the mixed run."""
    table = TS.classification_table(TS.MIXED_SIZES)
    print("\n" + TS.format_table(table))
    assert TS.cut_condition(table) == {path: (True, True) for path in TS.PATHS}
    lay = TS.layout_with(TS.MIXED_SIZES)
    tiles, total = O.make_tiles(lay)
    slices = TS.tile_slices(lay)
    fuser.set_tiles(lay)
    assert fuser.tile_elems == total
    nt = lay.ntiles
    resp = pf_synth.responses(pf_synth.seeds_for(B_WARP, 777), nt)
    for (pw, ph) in TS.PANOS:
        gt = _panoramas(pw, ph, B_WARP, 20261020)
        t_gt = _dev(gt)
        out = Guarded(B_WARP, total)
        fuser.warp_depth(t_gt, out.t, panofuse.make_responses(resp, DEV))
        got = out.host()
        assert not (got == SENTINEL).any(), "a tile pixel was not written"
        for b in CHECKED:
            ref = O.warp_depth(gt[b], tiles, total, O.responses(resp[b * nt:(b + 1) * nt]))
            assert np.array_equal(_bits(got[b]), _bits(ref)), (pw, ph, b, "response")
        plain = Guarded(B_WARP, total)
        fuser.warp_depth(t_gt, plain.t)
        got = plain.host()
        assert not (got == SENTINEL).any(), "a tile pixel was not written"
        for b in CHECKED:
            ref = O.warp_depth(gt[b], tiles, total, None)
            assert np.array_equal(_bits(got[b]), _bits(ref)), (pw, ph, b, "plain")
            gather = TS.warp_depth_gather(gt[b], lay)
            assert np.array_equal(_bits(got[b]), _bits(gather)), (pw, ph, b, "gather")
        for p in range(nt):
            fuser3.set_tiles(TS.one_tile(lay, p))
            n = slices[p].stop - slices[p].start
            solo = Guarded(B_WARP, n)
            fuser3.warp_depth(t_gt, solo.t)
            assert np.array_equal(_bits(solo.host()), _bits(got[:, slices[p]])), (pw, ph, p)


# ------------------------------------------------------------------------------------------
# 2. the smallest tiles
@pytest.mark.parametrize("pw,ph", [(512, 256), (302, 151)])
def test_warp_depth_smallest_tiles(fuser, pw, ph):
    lay = TS.layout_with(TS.SMALL_SIZES)
    tiles, total = O.make_tiles(lay)
    fuser.set_tiles(lay)  # >= 2 x 2 is the documented rule
    nt = lay.ntiles
    B = 3
    gt = _panoramas(pw, ph, B, 20261021)
    resp = pf_synth.responses(pf_synth.seeds_for(B, 778), nt)
    out = Guarded(B, total)
    fuser.warp_depth(_dev(gt), out.t, panofuse.make_responses(resp, DEV))
    got = out.host()
    plain = Guarded(B, total)
    fuser.warp_depth(_dev(gt), plain.t)
    got_plain = plain.host()
    for b in range(B):
        ref = O.warp_depth(gt[b], tiles, total, O.responses(resp[b * nt:(b + 1) * nt]))
        assert np.array_equal(_bits(got[b]), _bits(ref)), (b, "response")
        assert np.array_equal(_bits(got_plain[b]), _bits(O.warp_depth(gt[b], tiles, total))), b
        assert np.array_equal(_bits(got_plain[b]), _bits(TS.warp_depth_gather(gt[b], lay))), b


def test_set_tiles_rejects_a_one_wide_tile():
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected on a host without a GPU")
    f = panofuse.Fuser(0)
    for sizes in ([(1, 2)] + TS.SMALL_SIZES[1:], TS.SMALL_SIZES[:-1] + [(2, 1)]):
        with pytest.raises(panofuse.PanofuseError) as e:
            f.set_tiles(TS.layout_with(sizes))
        assert e.value.code == panofuse.PF_EINVAL
    f.set_tiles(TS.layout_with(TS.SMALL_SIZES))
    f.close()


# ------------------------------------------------------------------------------------------
# 3. the RGB warp, staged partial columns
def _warp_rgb(lay, pano):
    f = panofuse.Fuser(0)  # a new context builds the taps under the current setting
    f.set_tiles(lay)
    out = Guarded(pano.shape[0], TS.tile_elems(lay, 3), torch.uint8, 0xA5)
    f.warp_rgb(_dev(pano), out.t)
    got = out.host()
    f.close()
    return got


@pytest.mark.parametrize("pw,ph", [(512, 256), (1024, 512), (48, 24)])
def test_warp_rgb_partial_columns(pw, ph, monkeypatch):
    """Widths of 100, 68, 4, 132, 200, 40: multiples of 4, none of the 64-pixel patch, so the
    staged kernel (pw % 16 == 0) blends patches whose right lanes are outside the tile; 48 x 24
    wraps GL_REPEAT both ways and its footprints exceed ph / 2 (direct gathers).  The staged and
    the per-pixel kernel must equal each other on the whole batch and the oracle; with one width
    of 66 the whole layout takes the per-pixel kernel and must still equal the oracle."""
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected on a host without a GPU")
    rs = np.random.RandomState(pw + 7)
    pano = rs.randint(0, 256, size=(B_WARP, ph, pw, 3)).astype(np.uint8)
    pano[0, :, :, 0] = (np.arange(pw) * 255 // (pw - 1)).astype(np.uint8)[None, :]
    lay = TS.layout_with(TS.RGB_SIZES)
    tiles, _ = O.make_tiles(lay)
    outs = []
    for naive in ("0", "1"):
        monkeypatch.setenv("PF_WARP_RGB_NAIVE", naive)
        outs.append(_warp_rgb(lay, pano))
    assert np.array_equal(outs[0], outs[1])
    for b in (0, B_WARP - 1):
        assert np.array_equal(outs[0][b], O.warp_rgb(pano[b], tiles)), b
    monkeypatch.setenv("PF_WARP_RGB_NAIVE", "0")
    lay = TS.layout_with(TS.RGB_SIZES_UNALIGNED)
    tiles, _ = O.make_tiles(lay)
    got = _warp_rgb(lay, pano)
    for b in (0, B_WARP - 1):
        assert np.array_equal(got[b], O.warp_rgb(pano[b], tiles)), b


# ------------------------------------------------------------------------------------------
# 4. three channels through the pipeline
def _coeffs(n, ntiles, seed):
    rng = np.random.default_rng(seed)
    c = np.zeros((n, ntiles, 4), np.float32)
    c[:, :, 0] = rng.uniform(-0.3, 0.3, (n, ntiles))
    c[:, :, 1] = rng.uniform(-0.3, 0.3, (n, ntiles))
    c[:, :, 2] = rng.uniform(0.8, 1.2, (n, ntiles))
    c[:, :, 3] = rng.uniform(-0.05, 0.05, (n, ntiles))
    return c


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


def _out(w=OUT_W, h=None):
    return torch.zeros((BATCH, h or w // 2, w), dtype=torch.int16, device=DEV)


def _contexts(fuser, fuser3, lay):
    fuser.set_tiles(lay)
    fuser3.set_tiles(lay, channels=3)
    assert fuser3.tile_elems == 3 * fuser.tile_elems


def test_three_channel_warp_mixed_sizes(fuser, fuser3):
    """The warp's store offset g.off + i * g.c on the mixed layout, ragged and box staging."""
    lay = TS.layout_with(TS.MIXED_SIZES)
    _contexts(fuser, fuser3, lay)
    t3, n3 = O.make_tiles(lay, channels=3)
    nt = lay.ntiles
    resp = pf_synth.responses(pf_synth.seeds_for(BATCH, 779), nt)
    for (pw, ph) in TS.PANOS:
        gt = _panoramas(pw, ph, BATCH, 20261022)
        for r in (resp, None):
            dr = None if r is None else panofuse.make_responses(r, DEV)
            one = Guarded(BATCH, n3 // 3)
            fuser.warp_depth(_dev(gt), one.t, dr)
            three = Guarded(BATCH, n3, fill=float(TS.FILL))
            fuser3.warp_depth(_dev(gt), three.t, dr)
            got1, got3 = one.host(), three.host()
            assert np.array_equal(_bits(TS.channel(got3, 0)), _bits(got1)), (pw, ph)
            assert TS.fill_kept(got3), (pw, ph)
            for b in range(BATCH):
                rb = None if r is None else O.responses(r[b * nt:(b + 1) * nt])
                ref = TS.oracle_warp_filled(gt[b], t3, n3, rb)
                assert np.array_equal(_bits(got3[b]), _bits(ref)), (pw, ph, b)


@pytest.mark.parametrize("cfg", ["MIDAS", "LERES"])
def test_three_channel_warp(fuser, fuser3, cfg):
    k = TS.channel_case(cfg)
    lay, t3, n3, nt = k["lay"], k["t3"], k["n3"], k["lay"].ntiles
    _contexts(fuser, fuser3, lay)
    resp = np.concatenate([pf_synth.responses(pf_synth.seeds_for(1, 20261020 + 101 * s), nt)
                           for s in range(BATCH)])
    dr = panofuse.make_responses(resp, DEV)
    one = Guarded(BATCH, k["n1"])
    fuser.warp_depth(_dev(k["gts"]), one.t, dr)
    three = Guarded(BATCH, n3, fill=float(TS.FILL))
    fuser3.warp_depth(_dev(k["gts"]), three.t, dr)
    got1, got3 = one.host(), three.host()
    assert np.array_equal(_bits(got1), _bits(k["d1"]))
    assert np.array_equal(_bits(TS.channel(got3, 0)), _bits(got1)) and TS.fill_kept(got3)
    for b in range(BATCH):
        ref = TS.oracle_warp_filled(k["gts"][b], t3, n3, O.responses(resp[b * nt:(b + 1) * nt]))
        assert np.array_equal(_bits(got3[b]), _bits(ref)), b


@pytest.mark.parametrize("cfg", ["MIDAS", "LERES"])
def test_three_channel_tap_maps_and_audit(fuser, fuser3, cfg):
    k = TS.channel_case(cfg)
    _contexts(fuser, fuser3, k["lay"])
    t3, d3 = k["t3"], k["d3"][0]
    clamped = 0
    for level in range(O.num_levels(OUT_W)):
        lv = O.level_dims(OUT_W, OUT_W // 2, ZR, level)
        got1 = fuser.probe_taps(OUT_W, ZR, level).cpu().numpy()
        got3 = fuser3.probe_taps(OUT_W, ZR, level).cpu().numpy()
        assert np.array_equal(got3, np.where(got1 >= 0, got1 * 3, -1)), level
        assert np.array_equal(got3, O.probe_taps(t3, lv)), level
        _, n, oops, oob = O.targets(t3, d3, lv)
        clamped += oob
        want = {"w": lv.w, "h": lv.h, "h0": lv.h0, "h1": lv.h1, "taps_outside": oops,
                "taps_clamped": oob, "covered": int((n > 0).sum()),
                "uncovered_interior": int((n[lv.h0 + 1:lv.h1, 1:] == 0).sum()),
                "max_cover": int(n.max()), "seam": int(n[:, lv.w - 1].any())}
        a1, a3 = fuser.layout_audit(OUT_W, ZR, level), fuser3.layout_audit(OUT_W, ZR, level)
        print(f"{cfg} level {level}: {a3}")
        assert a3 == want, level
        assert {f: v for f, v in a1.items() if f != "taps_clamped"} == \
               {f: v for f, v in a3.items() if f != "taps_clamped"}
    assert clamped > 0  # the clamp to n - channels ran


@pytest.mark.parametrize("cfg", ["MIDAS", "LERES"])
def test_three_channel_register_merge_fuse(fuser, fuser3, cfg):
    k = TS.channel_case(cfg)
    lay, t3, nt = k["lay"], k["t3"], k["lay"].ntiles
    _contexts(fuser, fuser3, lay)
    t_emap = _dev(k["emaps"])

    # register(apply=True) with coefficients
    res = []
    for f, data in ((fuser, k["d1"]), (fuser3, k["d3"])):
        t = _dev(data)
        cf = torch.zeros((BATCH, nt, 4), dtype=torch.float32, device=DEV)
        c64 = torch.zeros((BATCH, nt, 4), dtype=torch.float64, device=DEV)
        f.register(t_emap, t, ZR, degree=3, apply=True, coeffs=cf, coeffs64=c64)
        f.synchronize()
        res.append((t.cpu().numpy(), cf.cpu().numpy(), c64.cpu().numpy()))
    (x1, cf1, c641), (x3, cf3, c643) = res
    assert np.array_equal(_bits(cf3), _bits(cf1)) and np.array_equal(_bits(c643), _bits(c641))
    assert np.array_equal(_bits(TS.channel(x3, 0)), _bits(x1)) and TS.fill_kept(x3)
    for b in range(BATCH):
        ref = k["d3"][b].copy()
        for p in range(nt):
            r64, rabcd, deg = O.register_tile(t3[p], k["d3"][b], k["emaps"][b], ZR)
            assert deg == 3
            assert np.array_equal(_bits(c643[b, p]), _bits(r64)), (b, p)
            assert np.array_equal(_bits(cf3[b, p]), _bits(rabcd)), (b, p)
            O.depth_to_depth(t3[p], ref, rabcd)
        assert np.array_equal(_bits(x3[b]), _bits(ref)), b

    # merge: tiles not modified
    refs = [O.merge(k["emaps"][b], t3, k["d3"][b].copy(), OUT_W, ZR) for b in range(BATCH)]
    merged = []
    for f, data in ((fuser, k["d1"]), (fuser3, k["d3"])):
        t, out = _dev(data), _out()
        cf = torch.zeros((BATCH, nt, 4), dtype=torch.float32, device=DEV)
        f.merge(t_emap, t, out, ZR, coeffs=cf)
        f.synchronize()
        assert np.array_equal(_bits(t.cpu().numpy()), _bits(data)), "merge must not modify tiles"
        merged.append((_u16(out), cf.cpu().numpy()))
    assert np.array_equal(merged[0][0], merged[1][0])
    assert np.array_equal(_bits(merged[0][1]), _bits(merged[1][1]))
    for b, (ref, abcd) in enumerate(refs):
        assert np.array_equal(_bits(merged[1][1][b]), _bits(abcd)), b
        assert np.array_equal(merged[1][0][b], ref), b
        assert int((ref != 0).sum()) > OUT_W

    # fuse with given coefficients: the transform inside the gather, tiles not modified
    given = _coeffs(BATCH, nt, 11)
    fused = []
    for f, data in ((fuser, k["d1"]), (fuser3, k["d3"])):
        t, out = _dev(data), _out()
        f.fuse(t_emap, t, out, ZR, coeffs=_dev(given))
        f.synchronize()
        assert np.array_equal(_bits(t.cpu().numpy()), _bits(data))
        fused.append(_u16(out))
    assert np.array_equal(fused[0], fused[1])
    for b in range(BATCH):
        d = k["d3"][b].copy()
        for p in range(nt):
            O.depth_to_depth(t3[p], d, given[b, p])
        assert TS.fill_kept(d)
        ref, _ = O.solve_depth_all(k["emaps"][b], t3, d, OUT_W, ZR)
        assert np.array_equal(fused[1][b], ref), b


@pytest.mark.parametrize("cfg", ["MIDAS", "LERES"])
def test_three_channel_stitch_and_smoothing(fuser, fuser3, cfg):
    k = TS.channel_case(cfg)
    lay, t3, nt = k["lay"], k["t3"], k["lay"].ntiles
    _contexts(fuser, fuser3, lay)
    given = _coeffs(BATCH, nt, 12)
    for cf in (None, given):
        got = []
        for f, data in ((fuser, k["d1"]), (fuser3, k["d3"])):
            t, out = _dev(data), _out()
            f.stitch(t, out, coeffs=None if cf is None else _dev(cf))
            f.synchronize()
            assert np.array_equal(_bits(t.cpu().numpy()), _bits(data))
            got.append(_u16(out))
        assert np.array_equal(got[0], got[1])
        for b in range(BATCH):
            ref = S.stitch(t3, k["d3"][b], OUT_W, OUT_W // 2, None if cf is None else cf[b])
            assert np.array_equal(got[1][b], ref), (b, cf is not None)
            assert int((ref != 0).sum()) > OUT_W
    for cf in (None, given):
        got = []
        for f, data in ((fuser, k["d1"]), (fuser3, k["d3"])):
            t, out = _dev(data), _out(256, 128)
            f.solve_smoothing(t, out, ZR, coeffs=None if cf is None else _dev(cf))
            f.synchronize()
            assert np.array_equal(_bits(t.cpu().numpy()), _bits(data))
            got.append(_u16(out))
        assert np.array_equal(got[0], got[1])
        for b in range(BATCH):
            d = k["d3"][b].copy()
            if cf is not None:
                for p in range(nt):
                    O.depth_to_depth(t3[p], d, cf[b, p])
            ref = O.solve_smoothing(t3, d, 256, 128, ZR)
            assert np.array_equal(got[1][b], ref), (b, cf is not None)
            assert int((ref != 0).sum()) > 256


def _to_disparity(data, tiles):
    """Per-tile normalised inverse depth (tests/test_gpu_layouts.py), 1-channel data."""
    out = np.empty_like(data)
    for t in tiles:
        n = t.width * t.height
        inv = np.float32(1.0) / np.maximum(data[t.offset:t.offset + n], np.float32(0.02))
        lo, hi = inv.min(), inv.max()
        out[t.offset:t.offset + n] = (inv - lo) / (hi - lo)
    return out


def test_three_channel_merge_disparity_midas(fuser, fuser3):
    """tests/test_gpu_layouts.py::test_merge_disparity_midas' comparison with interleaved tiles."""
    k = TS.channel_case("MIDAS")
    lay, t1, t3, nt = k["lay"], k["t1"], k["t3"], k["lay"].ntiles
    _contexts(fuser, fuser3, lay)
    disp1 = np.stack([_to_disparity(k["d1"][b], t1) for b in range(BATCH)])
    disp3 = TS.interleave(disp1)
    t_emap = _dev(k["emaps"])
    got = []
    for f, data in ((fuser, disp1), (fuser3, disp3)):
        t, out = _dev(data), _out()
        cf = torch.zeros((BATCH, nt, 4), dtype=torch.float32, device=DEV)
        f.merge_disparity(t_emap, t, out, ZR, coeffs=cf)
        f.synchronize()
        assert np.array_equal(_bits(t.cpu().numpy()), _bits(data))  # the caller's tiles stay
        got.append((_u16(out), cf.cpu().numpy()))
    assert np.array_equal(got[0][0], got[1][0])
    assert np.array_equal(_bits(got[0][1]), _bits(got[1][1]))
    for b in range(BATCH):
        xf = disp3[b].copy()
        for p, t in enumerate(t3):
            xs, ys, _, _ = O.reg_samples(t, disp3[b], k["emaps"][b], ZR)
            r64, _ = R.fit(xs, ys)
            abcd = r64.astype(np.float32)
            assert np.array_equal(_bits(got[1][1][b, p]), _bits(abcd)), (b, p)
            n = t.width * t.height * 3
            xf[t.offset:t.offset + n:3] = R.transform(disp3[b][t.offset:t.offset + n:3], abcd)
        assert TS.fill_kept(xf)
        want, _ = O.solve_depth_all(k["emaps"][b], t3, xf, OUT_W, ZR)
        assert np.array_equal(got[1][0][b], want), b
        assert int((want != 0).sum()) > OUT_W


# ------------------------------------------------------------------------------------------
# 5. mixed sizes through the fusion
def test_merge_mixed_sizes(fuser):
    """g.off and the per-tile sizes in the registration, the targets and the tap maps: the
    merge of six tiles of six sizes equals the oracle's in coefficients and u16."""
    lay = TS.layout_with(TS.MIXED_SIZES)
    tiles, total = O.make_tiles(lay)
    fuser.set_tiles(lay)
    emaps, datas = [], []
    for seed in range(BATCH):
        seeds = pf_synth.seeds_for(1, 20261020 + 101 * seed)
        emaps.append(pf_synth.baseline_emap(seeds, EW, EW // 2)[0].numpy())
        gt = pf_synth.scene_depth(seeds, OUT_W, OUT_W // 2)[0].numpy()
        resp = pf_synth.responses(seeds, lay.ntiles)
        datas.append(O.warp_depth(gt, tiles, total, O.responses(resp)))
    emaps, datas = np.stack(emaps), np.stack(datas)
    for level in range(O.num_levels(OUT_W)):
        lv = O.level_dims(OUT_W, OUT_W // 2, ZR, level)
        got = fuser.probe_taps(OUT_W, ZR, level).cpu().numpy()
        assert np.array_equal(got, O.probe_taps(tiles, lv)), level
    t_tiles, out = _dev(datas), _out()
    cf = torch.zeros((BATCH, lay.ntiles, 4), dtype=torch.float32, device=DEV)
    fuser.merge(_dev(emaps), t_tiles, out, ZR, coeffs=cf)
    fuser.synchronize()
    assert np.array_equal(_bits(t_tiles.cpu().numpy()), _bits(datas))
    got = _u16(out)
    for b in range(BATCH):
        ref, abcd = O.merge(emaps[b], tiles, datas[b].copy(), OUT_W, ZR)
        assert np.array_equal(_bits(cf.cpu().numpy()[b]), _bits(abcd)), b
        assert np.array_equal(got[b], ref), f"pano {b}: {int((got[b] != ref).sum())} pixels differ"
        assert int((ref != 0).sum()) > OUT_W
