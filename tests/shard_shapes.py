"""The sharded fusion's case table: the level and band calls of csrc/pf_shard.hip and the flows of
pf_dist (fuse_row_sharded, fuse_tile_sharded) at the sizes where kernels break.

tests/test_shard_shapes.py checks on the CPU, with the oracle, that every row is what it is listed
for; tests/test_gpu_shard_shapes.py runs the rows on the GPU.  A row:

  name, layout, out_w, out_h, zenith range, worlds, rep_levels, baseline, dims, sweeps

  layout      "c1" (6 tiles of 256^2), "holes" (test_fuse_shapes.holes_layout: no level has the
              coverage certificate, so every level takes the general form) or "edge"
              (test_gpu_targets_wave.edge_layout: eight tiles of six sizes, pixels covered four
              times, columns 0 and w - 1 uncovered)
  worlds      1; 2 (the C1 bands are dealt from the layout: tiles 0-2 are the upper zenith band);
              3 (two tiles per rank across the bands: the even split); 5; and 7 on C1 / 9 on the
              edge layout, where the last rank holds no tile (t0 == t1)
  rep_levels  0, 1 or "auto" (pf_dist.auto_rep_levels)
  baseline    index into test_fuse_shapes.BASELINES: none divides a level-0 width of its rows
  dims        (w, h, h0, h1) per level, asserted against pfo_level_dims
  sweeps      the levels on the per-sweep engine (jacobi_tcap < 1: no band passes; the sharded
              flow must replicate them)

What the sizes are for (all but 512x256 are rows of test_fuse_shapes.SHAPES):
  600x300    w % 4 = 2 at level 0 (the scalar form of the border kernel), w % 64 != 0 at every
             level (a partial patch column in the partial-sum kernel), odd level-0 height
  496x248    124 wide at level 0: the narrowest width with band passes
  504x252    126 wide: below 128
  440x220    level 0 on the per-sweep engine and without the certificate
  360x180    level 0 on the per-sweep engine, w % 64 = 26
  500x248    level 0 is 125 wide, an odd width (per-sweep), and the band passes of level 1 are
             seeded from the upsample of an odd-width level.  (500x250 has that level 0 too, but
             is no size the fusion takes: its level 1, 250x125, is not twice 125x62, and the
             oracle and pf_fuse both refuse it -- REFUSED_SIZE, asserted in the tests.)
  512x256    with ZR_ODD: bands of 47 / 91 / 179 rows (no multiple of 8), first rows 9 / 19 / 39
  1096x500, 1024x400   height != width / 2 (the bindings' out_h)
"""
import numpy as np

import pf_layouts as PL
import pf_synth
import pyoracle as O
import test_fuse_shapes as TS
from test_gpu_targets_wave import ZR_ODD, edge_layout

ZR = PL.ZENITH_RANGE
REPS = (0, 1, "auto")
PATCH_W, PATCH_H = 64, 8  # the partial-sum kernel's patch (kTPW x kTPH, csrc/pf_targets.hip)

_SHAPES = {(r[0], r[1]): r[2] for r in TS.SHAPES}


def _row(name, layout, w, h, zr, worlds, base, dims=None, sweeps=()):
    return dict(name=name, layout=layout, out_w=w, out_h=h, zr=zr, worlds=worlds, reps=REPS,
                baseline=TS.BASELINES[base], dims=dims or _SHAPES[(w, h)], sweeps=tuple(sweeps))


CASES = [
    _row("c1-600x300", "c1", 600, 300, ZR, (1, 2, 3, 5, 7), 1),
    _row("c1-496x248", "c1", 496, 248, ZR, (1, 2, 3), 0),
    _row("c1-504x252", "c1", 504, 252, ZR, (1, 2, 3), 2),
    _row("c1-440x220", "c1", 440, 220, ZR, (1, 2, 3), 1, sweeps=(0,)),
    _row("c1-360x180", "c1", 360, 180, ZR, (1, 2, 3), 0, sweeps=(0,)),
    _row("c1-500x248", "c1", 500, 248, ZR, (1, 2, 3), 2, sweeps=(0,)),
    _row("c1-512x256-odd", "c1", 512, 256, ZR_ODD, (1, 2, 3, 5, 7), 1,
         dims=((128, 64, 9, 55), (256, 128, 19, 109), (512, 256, 39, 217))),
    _row("c1-1096x500", "c1", 1096, 500, ZR, (1, 2, 3), 0),
    _row("c1-1024x400", "c1", 1024, 400, ZR, (1, 2, 3), 2),
    _row("holes-600x300", "holes", 600, 300, ZR, (1, 2, 3, 5), 0),
    _row("edge-512x256", "edge", 512, 256, ZR, (1, 2, 3, 5, 9), 1,
         dims=((128, 64, 9, 55), (256, 128, 18, 110), (512, 256, 36, 220))),
]
BY_NAME = {c["name"]: c for c in CASES}
# 125 wide at level 0 like 500x248, but its levels do not double: refused by the oracle and pf_fuse
REFUSED_SIZE = (500, 250)
# the side stream (HipRowShardBackend.enable_side): one case per layout
SIDE_CASES = ("c1-600x300", "holes-600x300", "edge-512x256")

LAYOUTS = {"c1": lambda: PL.config_layout("C1"), "holes": TS.holes_layout, "edge": edge_layout}
_INPUTS = {}


def nlevels(case):
    return O.num_levels(case["out_w"])


def level(case, lv):
    return O.level_dims(case["out_w"], case["out_h"], case["zr"], lv)


def engines(case, tiles, data):
    """[(engine, form)] per level: test_fuse_shapes.expected_engines' rules at the case's own
    zenith range."""
    res = []
    for lv in range(nlevels(case)):
        L = level(case, lv)
        _, cnt, _, _ = O.targets(tiles, data, L)
        cert = TS.has_certificate(cnt, L)
        engine = ("sweeps" if TS.tcap(L) < 1 else
                  "resident" if cert and TS.resident_blockings(L) else "streamed")
        res.append((engine, "packed" if cert else "general"))
    return res


def inputs(name):
    """A case's inputs, computed once and never written to: the layout, the oracle's tiles, the
    baseline, the tile data, the coefficients of the fused transform and the transformed data.
    The scene, responses and coefficients follow tests/test_gpu_targets_wave.py::_case (one
    panorama); the baseline has the row's size and channels (the channels past the first are
    noise)."""
    if name in _INPUTS:
        return _INPUTS[name]
    case = BY_NAME[name]
    lay = LAYOUTS[case["layout"]]()
    tiles, total = O.make_tiles(lay)
    seeds = pf_synth.seeds_for(1, 20261101 + len(name))
    ew, eh, ec = case["baseline"]
    emap = pf_synth.baseline_emap(seeds, ew, eh).numpy().astype(np.float32)[0]
    if ec > 1:
        rest = np.random.RandomState(len(name)).rand(eh, ew, ec - 1).astype(np.float32)
        emap = np.concatenate([emap[..., None], rest], -1)
    emap = np.ascontiguousarray(emap)
    gt = pf_synth.scene_depth(seeds, 512, 256).numpy()[0]
    resp = pf_synth.responses(seeds, lay.ntiles)
    data = O.warp_depth(gt, tiles, total, O.responses(resp))
    rng = np.random.default_rng(len(name))
    nt = lay.ntiles
    coeffs = np.zeros((nt, 4), np.float32)
    coeffs[:, 0] = rng.uniform(-0.3, 0.3, nt)
    coeffs[:, 1] = rng.uniform(-0.3, 0.3, nt)
    coeffs[:, 2] = rng.uniform(0.8, 1.2, nt)
    coeffs[:, 3] = rng.uniform(-0.05, 0.05, nt)
    xdata = data.copy()
    for p in range(nt):
        O.depth_to_depth(tiles[p], xdata, coeffs[p])
    for a in (emap, data, coeffs, xdata):
        a.setflags(write=False)
    _INPUTS[name] = dict(case=case, lay=lay, tiles=tiles, total=total, emap=emap, data=data,
                         coeffs=coeffs, xdata=xdata)
    return _INPUTS[name]


def reference(name):
    """The oracle's u16 panorama of the case (the transformed tiles fused), computed once."""
    k = inputs(name)
    if "ref" not in k:
        c = k["case"]
        ref, _ = O.solve_depth_all(k["emap"], k["tiles"], k["xdata"], c["out_w"], c["zr"],
                                   out_h=c["out_h"])
        ref.setflags(write=False)
        k["ref"] = ref
    return k["ref"]
