"""The per-wave targets gather (PF_TGT_WAVE=1, targets_wave in csrc/pf_targets.hip) against the
block form (PF_TGT_WAVE=0, targets_patch) and the CPU oracle, bit for bit.

The knob is read per call, so one context runs both forms on the same device buffers:

* the normalised target planes of pf_fuse_targets (k_targets_patch, one-panorama blocks) at every
  level, compared as int32 so that the NaN markers of uncovered pixels count;
* the whole fusion (k_targets_multi: groups of 8 panoramas, or one-panorama blocks at batch 1)
  as u16, knob 1 against knob 0 on the whole batch and against the oracle on its first and last
  panorama.

Shapes (the wave form owns a 64 x 8 patch per wave; lane 0's west and lane 63's east tap come
from the ring load):

* C1 (512 x 256, 6 tiles of 256^2);
* outputs 328 and 200 wide: the last patch column is partial at every level (320 and 192 are
  whole patches at the finest level), and level 0 of 200 is 50 wide, less than one patch;
* zenith bands whose row count is no multiple of 8, and bands that start at an odd row (the
  cases' level tables are asserted, not assumed);
* batches of 1, 3 and 9: one-panorama blocks, a partial group, a full group plus a tail of one;
* the tile-edge layout (edge_layout): eight tiles of six sizes, none a multiple of the patch,
  whose boxes at the finest level begin exactly at a patch's first column and end exactly at a
  patch's last one, overlap so that pixels are covered by four tiles, and leave columns 0 and
  w - 1 (and the patches around them) uncovered;
* with the fused transform (coeffs) and without.

One case runs under the validity rule: those kernels have the block form only and ignore the
knob, so both settings must give the same planes and the same fusion.
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import panofuse  # noqa: E402
import pf_layouts as PL  # noqa: E402
import pf_synth  # noqa: E402
import pyoracle as O  # noqa: E402

DEV = "cuda:0"
ZR = PL.ZENITH_RANGE
ZR_ODD = (PL.f32(PL.D2R(27.5)), PL.f32(PL.D2R(152.0)))
PATCH_W, PATCH_H = 64, 8


@pytest.fixture(scope="module")
def fuser():
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected on a host without a GPU")
    f = panofuse.Fuser(0)
    yield f
    f.close()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def edge_layout():
    """Two zenith bands of four 110-degree windows; the ranges are set in columns of the 512-wide
    finest level (a box runs from round(range0 / 2pi * 511) down to, and excluding,
    round(range1 / 2pi * 511)): columns [64, 135], [120, 255], [250, 390], [380, 500] per sector,
    and the upper band's rows reach 6 degrees into the lower band's."""
    lay = PL.band_layout(4, 2, 96, 80, 10, 24, "edge4x2")
    cols = [(64, 135), (120, 255), (250, 390), (380, 500)]
    for p in range(lay.ntiles):
        lo, hi = cols[p % 4]
        lay.ranges[p, 0] = PL.f32(hi * (2 * PL.MYPI) / 511)
        lay.ranges[p, 1] = PL.f32((lo - 1) * (2 * PL.MYPI) / 511)
        if p < 4:
            lay.ranges[p, 3] = PL.f32(PL.D2R(96.0))
    sizes = [(100, 70), (65, 33), (63, 31), (130, 97), (200, 50), (40, 20), (96, 80), (70, 90)]
    lay.tile_w = np.array([s[0] for s in sizes], np.int32)
    lay.tile_h = np.array([s[1] for s in sizes], np.int32)
    return lay


def _boxes(tiles, lv):
    """Per tile the columns [lo, hi] and rows [y0, y1] of its box (oracle/pf_oracle.c)."""
    out = []
    for t in tiles:
        v = [C.c_int(0) for _ in range(5)]
        rc = O.lib().pfo_tile_box(C.byref(t), C.byref(lv), *[C.byref(x) for x in v])
        assert rc == 0
        x0, x1, y0, y1, xs = (x.value for x in v)
        out.append((x0, x1 - 1, y0, y1) if xs > 0 else (x1 + 1, x0, y0, y1))
    return out


# name: (layout, output width, zenith range, batch, fused transform)
CASES = {
    "c1": (lambda: PL.config_layout("C1"), 512, ZR, 3, True),
    "c1-plain": (lambda: PL.config_layout("C1"), 512, ZR, 3, False),
    "c1-odd-band-b9": (lambda: PL.config_layout("C1"), 512, ZR_ODD, 9, True),
    "w328-b9": (lambda: PL.config_layout("C1"), 328, ZR, 9, True),
    "w200-b1": (lambda: PL.config_layout("C1"), 200, ZR, 1, True),
    "w200-b1-plain": (lambda: PL.config_layout("C1"), 200, ZR, 1, False),
    "edge-b3": (edge_layout, 512, ZR, 3, True),
    "edge-b9-plain": (edge_layout, 512, ZR_ODD, 9, False),
    "edge-b1": (edge_layout, 512, ZR_ODD, 1, True),
}
_INPUTS = {}


def _case(name):
    """The case's inputs, computed once: layout, oracle tiles, baselines, tile data, coefficients."""
    if name in _INPUTS:
        return _INPUTS[name]
    mk, out_w, zr, B, xform = CASES[name]
    lay = mk()
    tiles, total = O.make_tiles(lay)
    seeds = pf_synth.seeds_for(B, 20261101 + len(name))
    emaps = pf_synth.baseline_emap(seeds, 128, 64).numpy()
    gts = pf_synth.scene_depth(seeds, 512, 256).numpy()
    resp = pf_synth.responses(seeds, lay.ntiles)
    nt = lay.ntiles
    datas = np.stack([O.warp_depth(gts[b], tiles, total, O.responses(resp[b * nt:(b + 1) * nt]))
                      for b in range(B)])
    coeffs = None
    if xform:
        rng = np.random.default_rng(len(name))
        coeffs = np.zeros((B, nt, 4), np.float32)
        coeffs[:, :, 0] = rng.uniform(-0.3, 0.3, (B, nt))
        coeffs[:, :, 1] = rng.uniform(-0.3, 0.3, (B, nt))
        coeffs[:, :, 2] = rng.uniform(0.8, 1.2, (B, nt))
        coeffs[:, :, 3] = rng.uniform(-0.05, 0.05, (B, nt))
    _INPUTS[name] = dict(lay=lay, tiles=tiles, total=total, out_w=out_w, zr=zr, B=B, emaps=emaps,
                         datas=datas, coeffs=coeffs)
    return _INPUTS[name]


def test_case_shapes():
    """What the cases are chosen for holds: partial patch columns, band rows that are no multiple
    of the patch height, bands starting at odd rows, and the tile-edge layout's boxes."""
    fin = {n: O.level_dims(c[1], c[1] // 2, c[2], 2) for n, c in CASES.items()}
    for w in (328, 200):
        assert all(O.level_dims(w, w // 2, ZR, level).w % PATCH_W for level in range(3)), w
    assert O.level_dims(200, 100, ZR, 0).w < PATCH_W
    for name in ("c1", "c1-odd-band-b9", "w328-b9", "w200-b1", "edge-b1"):
        assert (fin[name].h1 - fin[name].h0 + 1) % PATCH_H, name
    for name in ("c1-odd-band-b9", "w328-b9", "edge-b1"):
        assert fin[name].h0 % 2 == 1, name
    k = _case("edge-b3")
    lv = fin["edge-b3"]
    boxes = _boxes(k["tiles"], lv)
    assert any(lo % PATCH_W == 0 for lo, _, _, _ in boxes)           # lane 0's W: a ring value
    assert any(hi % PATCH_W == PATCH_W - 1 for _, hi, _, _ in boxes)  # lane 63's E: a ring value
    assert all(lo >= 1 and hi <= lv.w - 2 for lo, hi, _, _ in boxes)
    _, n, _, _ = O.targets(k["tiles"], k["datas"][0], lv)
    assert n.max() == 4 and not n[:, 0].any() and not n[:, lv.w - 1].any()
    assert (n[lv.h0 + 1:lv.h1, 64] > 0).any() and (n[lv.h0 + 1:lv.h1, 255] > 0).any()


def _planes(fuser, k, monkeypatch, b=0):
    """Per knob setting, every level's target plane of panorama b as int32."""
    t_tiles = _dev(k["datas"][b])
    cf = None if k["coeffs"] is None else _dev(k["coeffs"][b])
    out = {}
    for knob in ("0", "1"):
        monkeypatch.setenv("PF_TGT_WAVE", knob)
        planes = []
        for level in range(O.num_levels(k["out_w"])):
            lv = O.level_dims(k["out_w"], k["out_w"] // 2, k["zr"], level)
            ln = torch.full((lv.h * lv.w,), -3.0, dtype=torch.float32, device=DEV)
            fuser.fuse_targets(t_tiles, cf, k["out_w"], k["zr"], level, ln)
            fuser.synchronize()
            planes.append(ln.cpu().numpy().view(np.int32).reshape(lv.h, lv.w))
        out[knob] = planes
    return out


def _fused(fuser, k, monkeypatch):
    """Per knob setting, the fusion's u16 output of the whole batch."""
    t_emap, t_tiles = _dev(k["emaps"]), _dev(k["datas"])
    cf = None if k["coeffs"] is None else _dev(k["coeffs"])
    out = {}
    for knob in ("0", "1"):
        monkeypatch.setenv("PF_TGT_WAVE", knob)
        o = torch.zeros((k["B"], k["out_w"] // 2, k["out_w"]), dtype=torch.int16, device=DEV)
        fuser.fuse(t_emap, t_tiles, o, k["zr"], coeffs=cf)
        fuser.synchronize()
        out[knob] = o.cpu().numpy().view(np.uint16)
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_planes_bit_for_bit(fuser, name, monkeypatch):
    k = _case(name)
    fuser.set_tiles(k["lay"])
    p = _planes(fuser, k, monkeypatch, b=k["B"] - 1)
    for level, (a, w) in enumerate(zip(p["0"], p["1"])):
        bad = int((a != w).sum())
        assert bad == 0, f"{name} level {level}: {bad} target words differ"
        lv = O.level_dims(k["out_w"], k["out_w"] // 2, k["zr"], level)
        band = w[lv.h0:lv.h1 + 1]
        assert (band != np.float32(-3.0).view(np.int32)).all(), "a band pixel was not written"


@pytest.mark.parametrize("name", list(CASES))
def test_fusion_equals_block_form_and_oracle(fuser, name, monkeypatch):
    k = _case(name)
    fuser.set_tiles(k["lay"])
    got = _fused(fuser, k, monkeypatch)
    assert np.array_equal(got["1"], got["0"]), f"{int((got['1'] != got['0']).sum())} pixels differ"
    for b in sorted({0, k["B"] - 1}):
        d = k["datas"][b].copy()
        if k["coeffs"] is not None:
            for p in range(k["lay"].ntiles):
                O.depth_to_depth(k["tiles"][p], d, k["coeffs"][b, p])
        ref, _ = O.solve_depth_all(k["emaps"][b], k["tiles"], d, k["out_w"], k["zr"])
        assert np.array_equal(got["1"][b], ref), f"pano {b}: {int((got['1'][b] != ref).sum())}"
        assert int((ref != 0).sum()) > k["out_w"]


def test_validity_rule_ignores_the_knob(fuser, monkeypatch):
    """Tiles with invalid pixels (NaN, and holes written as 0) under set_tile_validity(lo=0): the
    masked kernels give the same planes and the same fusion at either knob setting."""
    k = dict(_case("edge-b3"))
    datas = k["datas"].copy()
    rng = np.random.default_rng(7)
    holes = rng.random(datas.shape) < 0.02
    datas[holes] = np.where(rng.random(int(holes.sum())) < 0.5, np.float32("nan"), np.float32(0))
    k["datas"] = datas
    fuser.set_tiles(k["lay"])
    fuser.set_tile_validity(lo=0.0)
    try:
        p = _planes(fuser, k, monkeypatch)
        got = _fused(fuser, k, monkeypatch)
    finally:
        fuser.set_tile_validity()
    for level, (a, w) in enumerate(zip(p["0"], p["1"])):
        assert np.array_equal(a, w), level
    assert np.array_equal(got["1"], got["0"])
    assert int((got["1"] != 0).sum()) > k["out_w"]
