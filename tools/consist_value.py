"""What the overlap-consistent registration buys, on the CPU with fixed seeds.

Per config (C1: 6 tiles of 256^2, 512 x 256; C2: 20 tiles of 512^2, 2048 x 1024) the default-seed
pf_synth scene is warped into the tiles, every tile is toned by its own curve
v = (0.8 + 0.05 (p mod 3)) z^(1.1 - 0.05 (p mod 2)) + 0.03, and the tiles are registered over the
blurred baseline with lambda in {0, 0.25, 1, 4} by the restatement of tests/consist_ref.py (its
fp64 pair table; lambda = 0 is the independent least squares).  Per lambda it prints

  overlap rms   sqrt(sum d^2 / n) of the transformed values over all pair samples
  seam          mean |a - b| / 65535 of the direct stitch over neighbouring pixels (4-neighbourhood)
                that take their value from different tiles
  band error    mean |out / 65535 - gt| of the fused panorama over the band

It reports; no target is set.  Usage: python tools/consist_value.py [C1] [C2]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("tests", "oracle", "wacv2023-high-resolution-depth-estimation-for-panoramas-through-"
                               "perspective-map-registrations_amd"):
    sys.path.insert(0, os.path.join(ROOT, sub))

import consist_ref as CR  # noqa: E402
import pf_layouts as PL  # noqa: E402
import pf_synth  # noqa: E402
import pyoracle as O  # noqa: E402
import stitch_ref as SR  # noqa: E402

ZR = PL.ZENITH_RANGE
f32 = np.float32


def tone(z, p):
    return ((0.8 + 0.05 * (p % 3)) * z.astype(np.float64) ** (1.1 - 0.05 * (p % 2)) + 0.03
            ).astype(f32)


def seam(out, first):
    o = out.astype(np.float64) / 65535.0
    tot, n = 0.0, 0
    for a, b, fa, fb in ((o[:, :-1], o[:, 1:], first[:, :-1], first[:, 1:]),
                         (o[:-1], o[1:], first[:-1], first[1:])):
        sel = (fa != fb) & (fa >= 0) & (fb >= 0)
        tot += float(np.abs(a - b)[sel].sum())
        n += int(sel.sum())
    return tot / n


def run(cfg):
    lay = PL.config_layout(cfg)
    ow, ew = PL.CONFIGS["C2" if cfg == "C2" else cfg]
    oh = ow // 2
    seeds = pf_synth.seeds_for(1)
    emap = pf_synth.baseline_emap(seeds, ew, ew // 2)[0].numpy()
    gt = pf_synth.scene_depth(seeds, ow, oh)[0].numpy()
    tiles, total = O.make_tiles(lay)
    ray = O.warp_depth(gt, tiles, total)
    data = np.empty_like(ray)
    for p, t in enumerate(tiles):
        s = slice(t.offset, t.offset + t.width * t.height)
        data[s] = tone(ray[s], p)
    pairs, index = CR.pair_table64(lay, ZR)
    values = CR.pair_values(CR.tile_offsets(lay), data, pairs, index)
    D = [CR.data_sums(*O.reg_samples(t, data, emap, ZR)[:2]) for t in tiles]
    Pm = [CR.pair_sums(vp, vq) for vp, vq in values]
    _, first = SR.cover(tiles, ow, oh)
    lv = O.level_dims(ow, oh, ZR, O.num_levels(ow) - 1)
    print(f"{cfg}: {lay.ntiles} tiles, {len(pairs)} pairs, {len(index)} pair samples")
    for lam in (0.0, 0.25, 1.0, 4.0):
        c64, sm = CR.register(D, Pm, pairs, lam)
        cf = c64.astype(f32)
        rms = CR.overlap_rms(CR.overlap_stats(values, pairs, cf))
        st = SR.stitch(tiles, data, ow, oh, cf)
        fixed = data.copy()
        for p, t in enumerate(tiles):
            O.depth_to_depth(t, fixed, cf[p])
        out, _ = O.solve_depth_all(emap, tiles, fixed, ow, ZR)
        err = float(np.mean(np.abs(out.astype(np.float64) / 65535.0 - gt)[lv.h0:lv.h1 + 1]))
        print(f"  lambda {lam:<5g} overlap rms {rms:.5f}  seam {seam(st, first):.5f}  "
              f"band error {err:.5f}  data cost {sm[0]:.4f}  pair cost {sm[1]:.4f}", flush=True)
    print(f"  (the scene itself across the same seams: {seam((gt * 65535).astype(np.uint16), first):.5f})")


if __name__ == "__main__":
    for name in (sys.argv[1:] or ["C1", "C2"]):
        run(name)
