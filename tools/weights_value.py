"""What per-pixel tile weights cost and what they buy, on the GPU.

cost    At C3 (batch 64, 2048 x 1024, 20 tiles of 512^2) and C1 (batch 1, 512 x 256, 6 tiles of
        256^2), alternating in one process: merge_weighted with the tent (one shared set),
        merge_weighted with one smooth field per panorama, merge under
        set_tile_validity(-inf, inf) (the same general Jacobi passes: the yardstick) and the
        plain merge (for scale).  Per variant the median device-event time of a call and the
        per-stage times of profile_read, in a pass of its own.
effect  On the 6 toned 256^2 tiles of tools/consist_value.py (C1, default seed): the band error
        against the ground truth, the overlap rms of pf_overlap_stats and the stitch seam, for the
        plain merge against the tent merge; again with tile noise whose sigma grows linearly
        toward the tile border; and with a corrupted rectangle that has weight 0 in one panorama
        of a batch of two only.

It reports; no target is set.  Usage: python tools/weights_value.py [cost] [effect] [--out FILE]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("tests", "oracle", "wacv2023-high-resolution-depth-estimation-for-panoramas-through-"
                               "perspective-map-registrations_amd"):
    sys.path.insert(0, os.path.join(ROOT, sub))

import panofuse  # noqa: E402
import pf_layouts as PL  # noqa: E402
import pf_synth  # noqa: E402
import pyoracle as O  # noqa: E402
import stitch_ref as SR  # noqa: E402
import weight_ref as WR  # noqa: E402
from consist_value import seam, tone  # noqa: E402

ZR = PL.ZENITH_RANGE
DEV = "cuda:0"
f32 = np.float32
INF = float("inf")


def smooth_fields(tiles, n, seed=20261021):
    """n weight sets in [0.1, 1]: per tile an 8 x 8 grid, upsampled bilinearly."""
    rs = np.random.RandomState(seed)
    total = sum(t.width * t.height for t in tiles)
    out = np.empty((n, total), f32)
    for t in tiles:
        w, h = t.width, t.height
        g = 0.1 + 0.9 * rs.rand(n, 8, 8)
        ys, xs = np.linspace(0, 7, h), np.linspace(0, 7, w)
        y0, x0 = np.minimum(ys.astype(int), 6), np.minimum(xs.astype(int), 6)
        fy, fx = (ys - y0)[None, :, None], (xs - x0)[None, None, :]
        v = ((1 - fy) * (1 - fx) * g[:, y0][:, :, x0] + (1 - fy) * fx * g[:, y0][:, :, x0 + 1]
             + fy * (1 - fx) * g[:, y0 + 1][:, :, x0] + fy * fx * g[:, y0 + 1][:, :, x0 + 1])
        out[:, t.offset:t.offset + w * h] = v.reshape(n, -1).astype(f32)
    return out


# ---- cost ---------------------------------------------------------------------------------------
def cost_config(cfg, batch, steps, warmup):
    lay = PL.config_layout(cfg)
    ow, ew = PL.CONFIGS["C2" if cfg == "C3" else cfg]  # C3 is C2's shape at batch 64
    tiles, total = O.make_tiles(lay)
    nscene = min(batch, 4)  # distinct scenes, repeated over the batch
    emaps, datas = [], []
    for k in range(nscene):
        seeds = pf_synth.seeds_for(1, 90000 + k)
        gt = pf_synth.scene_depth(seeds, ow, ow // 2)[0].numpy()
        emaps.append(pf_synth.baseline_emap(seeds, ew, ew // 2)[0].numpy())
        datas.append(O.warp_depth(gt, tiles, total,
                                  O.responses(pf_synth.responses(seeds, lay.ntiles))))
    idx = [b % nscene for b in range(batch)]
    t_emap = torch.from_numpy(np.stack([emaps[i] for i in idx])).to(DEV).contiguous()
    t_tiles = torch.from_numpy(np.stack([datas[i] for i in idx])).to(DEV).contiguous()
    fields = smooth_fields(tiles, nscene)
    t_field = torch.from_numpy(np.stack([fields[i] for i in idx])).to(DEV).contiguous()
    out = torch.zeros((batch, ow // 2, ow), dtype=torch.int16, device=DEV)
    cf = torch.zeros((batch, lay.ntiles, 4), dtype=torch.float32, device=DEV)

    plain = panofuse.Fuser(0)
    plain.set_tiles(lay)
    masked = panofuse.Fuser(0)
    masked.set_tiles(lay)
    masked.set_tile_validity(-INF, INF)
    t_tent = plain.tent_weights()
    variants = {
        "weighted tent (wbatch 1)": (plain, lambda fz: fz.merge_weighted(t_emap, t_tiles, t_tent,
                                                                         out, ZR, coeffs=cf)),
        f"weighted field (wbatch {batch})": (plain, lambda fz: fz.merge_weighted(
            t_emap, t_tiles, t_field, out, ZR, coeffs=cf)),
        "validity rule (-inf, inf)": (masked, lambda fz: fz.merge(t_emap, t_tiles, out, ZR,
                                                                  coeffs=cf)),
        "plain merge": (plain, lambda fz: fz.merge(t_emap, t_tiles, out, ZR, coeffs=cf)),
    }
    for fz, call in variants.values():
        for _ in range(warmup):
            call(fz)
        fz.synchronize()
    times = {k: [] for k in variants}
    for _ in range(steps):  # alternating, so drift hits every variant alike
        for name, (fz, call) in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(fz.stream)
            call(fz)
            b.record(fz.stream)
            fz.synchronize()
            times[name].append(a.elapsed_time(b))
    res = {}
    for name, (fz, call) in variants.items():  # the stages, in a pass of their own
        fz.profile(True)
        for _ in range(steps):
            call(fz)
        fz.synchronize()
        st = fz.profile_read()
        fz.profile(False)
        t = np.array(times[name])
        res[name] = {"call_ms_median": float(np.median(t)), "call_ms_min": float(t.min()),
                     "call_ms_max": float(t.max()),
                     "stage_ms": {k: v[0] / steps for k, v in st.items() if v[2]},
                     "stage_launches": {k: v[2] // steps for k, v in st.items() if v[2]}}
    print(f"{cfg} batch {batch}: {lay.ntiles} tiles, {ow} x {ow // 2}, {steps} calls each")
    for name, r in res.items():
        stages = "  ".join(f"{k} {v:.3f}" for k, v in r["stage_ms"].items())
        print(f"  {name:<28} call {r['call_ms_median']:.3f} ms (min {r['call_ms_min']:.3f}, max "
              f"{r['call_ms_max']:.3f})  stages: {stages}", flush=True)
    return res


# ---- effect -------------------------------------------------------------------------------------
def effect():
    lay = PL.config_layout("C1")
    ow, ew = PL.CONFIGS["C1"]
    oh = ow // 2
    seeds = pf_synth.seeds_for(1)
    emap = pf_synth.baseline_emap(seeds, ew, ew // 2)[0].numpy()
    gt = pf_synth.scene_depth(seeds, ow, oh)[0].numpy()
    tiles, total = O.make_tiles(lay)
    ray = O.warp_depth(gt, tiles, total)
    toned = np.empty_like(ray)
    for p, t in enumerate(tiles):
        s = slice(t.offset, t.offset + t.width * t.height)
        toned[s] = tone(ray[s], p)
    tent = WR.tent(tiles)
    rs = np.random.RandomState(7)
    # noise whose sigma grows linearly toward the tile border: 0 at the tent's top, 0.05 at the rim
    noisy = (toned + (0.05 * (1.0 - tent) * rs.randn(total)).astype(f32)).astype(f32)
    corrupt = toned.copy()  # a rectangle of tile 0 replaced by a constant
    c0 = corrupt[:256 * 256].reshape(256, 256)
    c0[100:, 100:180] = 0.9
    zero_rect = np.ones(total, f32)
    zero_rect[:256 * 256].reshape(256, 256)[100:, 100:180] = 0.0
    _, first = SR.cover(tiles, ow, oh)
    lv = O.level_dims(ow, oh, ZR, O.num_levels(ow) - 1)
    fz = panofuse.Fuser(0)
    fz.set_tiles(lay)

    def measure(data, weights):
        """[(band error, overlap rms, seam)] per panorama of data [B][total]; weights None: the
        plain merge, else [total] or [B][total]."""
        B = data.shape[0]
        t_emap = torch.from_numpy(np.stack([emap] * B)).to(DEV).contiguous()
        t = torch.from_numpy(data).to(DEV).contiguous()
        out = torch.zeros((B, oh, ow), dtype=torch.int16, device=DEV)
        st = torch.zeros((B, oh, ow), dtype=torch.int16, device=DEV)
        cf = torch.zeros((B, lay.ntiles, 4), dtype=torch.float32, device=DEV)
        if weights is None:
            fz.merge(t_emap, t, out, ZR, coeffs=cf)
        else:
            fz.merge_weighted(t_emap, t, torch.from_numpy(weights).to(DEV).contiguous(), out, ZR,
                              coeffs=cf)
        stats = fz.overlap_stats(t, ZR, coeffs=cf)
        fz.stitch(t, st, cf)
        fz.synchronize()
        o = out.cpu().numpy().view(np.uint16)
        s = stats.cpu().numpy()
        rows = []
        for b in range(B):
            err = float(np.mean(np.abs(o[b].astype(np.float64) / 65535.0 - gt)[lv.h0:lv.h1 + 1]))
            rms = float(np.sqrt(s[b, :, 2].sum() / s[b, :, 0].sum()))
            rows.append((err, rms, seam(st.cpu().numpy().view(np.uint16)[b], first)))
        return rows

    res = {}

    def report(name, rows):
        res[name] = [{"band_error": r[0], "overlap_rms": r[1], "seam": r[2]} for r in rows]
        for b, r in enumerate(rows):
            print(f"  {name:<44} pano {b}: band error {r[0]:.5f}  overlap rms {r[1]:.5f}  "
                  f"seam {r[2]:.5f}", flush=True)

    print("effect: C1, 6 toned 256^2 tiles")
    report("toned, plain", measure(toned[None], None))
    report("toned, tent", measure(toned[None], tent))
    report("border noise, plain", measure(noisy[None], None))
    report("border noise, tent", measure(noisy[None], tent))
    pair = np.stack([corrupt, toned])
    report("corrupt rectangle in pano 0, plain", measure(pair, None))
    report("corrupt rectangle, weight 0 in pano 0 only",
           measure(pair, np.stack([zero_rect, np.ones(total, f32)])))
    return res


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    outfile = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    args = [a for a in args if a != outfile] or ["cost", "effect"]
    if not torch.cuda.is_available():
        raise SystemExit("weights_value needs a GPU: nothing is measured without one")
    result = {}
    if "effect" in args:
        result["effect"] = effect()
    if "cost" in args:
        result["cost"] = {"C1": cost_config("C1", 1, 50, 5), "C3": cost_config("C3", 64, 10, 3)}
    if outfile:
        with open(outfile, "w") as f:
            json.dump(result, f, indent=1)
