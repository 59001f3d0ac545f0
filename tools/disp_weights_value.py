"""What per-pixel weights for disparity tiles cost and what they buy, on the GPU (DESIGN.md
section 13).

cost    At the C3 shape (64 panoramas x 20 tiles of 512^2 x 2,409 samples, a 512 x 256 baseline,
        2048 x 1024 output), alternating call by call in one process on the same buffers:
        register_disparity (the untouched kernel: the yardstick), register_disparity_weighted with
        one weight set (the tent, wbatch 1) and with one set per panorama (wbatch 64).  Device
        events around --inner back-to-back calls, the median with min - max over --runs windows.
        Then merge_disparity against merge_disparity_weighted, whole calls alternating, and their
        per-stage times from profile_read in a pass of their own.
value   The disparity tiles of the default pf_synth scene at C1 (6 tiles of 256^2, 512 x 256),
        with the part of every tile above zenith --sky (a fraction of pi; 0.40 by default) set to
        disparity 0, what a network writes for sky; the baseline is unchanged.  The band error
        (mean |result - ground truth| over the band rows of the last level), overall and over the
        rows below the sky line, for four fits: unweighted, range:0:inf, Huber at --huber (the tool
        that exists without weights), and the clean tiles.

It reports; no target is set.
Usage: python tools/disp_weights_value.py [cost] [value] [--out FILE] [--runs 9] [--inner 10]"""
import argparse
import json
import os
import statistics
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

ZR = PL.ZENITH_RANGE
DEV = torch.device("cuda:0")
INF = float("inf")


def disparity_tiles(fz, lay, seeds, out_w):
    """[B][tile_elems] per-tile normalised inverse depth of the warped scene (MiDaS' convention),
    on the device."""
    B = len(seeds)
    gt = pf_synth.scene_depth(seeds, out_w, out_w // 2, device=DEV).contiguous()
    depth = torch.zeros((B, fz.tile_elems), dtype=torch.float32, device=DEV)
    fz.warp_depth(gt, depth, panofuse.make_responses(pf_synth.responses(seeds, lay.ntiles), DEV))
    fz.synchronize()
    inv = 1.0 / depth.view(B, lay.ntiles, -1).clamp(min=0.02)
    lo, hi = inv.amin(dim=2, keepdim=True), inv.amax(dim=2, keepdim=True)
    return ((inv - lo) / (hi - lo)).reshape(B, -1).contiguous(), gt


def timed(fz, calls, runs, warmup, inner):
    """{name: [ms per call]}: the calls alternate window by window of `inner` calls."""
    times = {name: [] for name in calls}
    for i in range(warmup + runs):
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(fz.stream)
            for _ in range(inner):
                fn()
            e1.record(fz.stream)
            e1.synchronize()
            if i >= warmup:
                times[name].append(e0.elapsed_time(e1) / inner)
    return times


def stats(t):
    return {"median_ms": round(statistics.median(t), 5), "min_ms": round(min(t), 5),
            "max_ms": round(max(t), 5)}


def cost(runs, warmup, inner, batch=64):
    lay = PL.config_layout("C3")
    out_w, ew = 2048, 512
    fz = panofuse.Fuser(0)
    fz.set_tiles(lay)
    seeds = pf_synth.seeds_for(batch)
    emap = pf_synth.baseline_emap(seeds, ew, ew // 2, device=DEV).contiguous()
    tiles, _ = disparity_tiles(fz, lay, seeds, out_w)
    nt = lay.ntiles
    cf = torch.zeros((batch, nt, 4), dtype=torch.float32, device=DEV)
    tent = fz.tent_weights()
    gen = torch.Generator(device=DEV).manual_seed(20261021)
    field = (0.1 + 0.9 * torch.rand((batch, fz.tile_elems), generator=gen, device=DEV,
                                    dtype=torch.float32)).contiguous()
    out = torch.zeros((batch, out_w // 2, out_w), dtype=torch.int16, device=DEV)
    reg = {
        "register_disparity": lambda: fz.register_disparity(emap, tiles, ZR, apply=False,
                                                            coeffs=cf),
        "register_disparity_weighted wbatch 1": lambda: fz.register_disparity_weighted(
            emap, tiles, tent, ZR, apply=False, coeffs=cf),
        f"register_disparity_weighted wbatch {batch}": lambda: fz.register_disparity_weighted(
            emap, tiles, field, ZR, apply=False, coeffs=cf),
    }
    res = {"shape": {"batch": batch, "tiles": nt, "samples_per_tile": 2409}, "runs": runs,
           "inner_calls": inner, "register": {}, "merge": {}}
    base = None
    for name, t in timed(fz, reg, runs, warmup, inner).items():
        res["register"][name] = stats(t)
        base = base or res["register"][name]["median_ms"]
        res["register"][name]["ratio"] = round(res["register"][name]["median_ms"] / base, 3)
        print(f"  {name:<44} {res['register'][name]}", flush=True)
    sm = torch.zeros((batch, nt, 6), dtype=torch.float64, device=DEV)
    fz.register_disparity_weighted(emap, tiles, tent, ZR, apply=False, summary=sm)
    fz.synchronize()
    its = sm.cpu().numpy()[..., 2]
    res["lm_iterations_tent"] = {"min": int(its.min()), "median": float(np.median(its)),
                                 "max": int(its.max())}
    mrg = {
        "merge_disparity": lambda: fz.merge_disparity(emap, tiles, out, ZR, coeffs=cf),
        "merge_disparity_weighted wbatch 1": lambda: fz.merge_disparity_weighted(
            emap, tiles, tent, out, ZR, coeffs=cf),
    }
    for name, t in timed(fz, mrg, max(3, runs // 2), 1, 1).items():
        res["merge"][name] = stats(t)
    for name, fn in mrg.items():  # the stages, in a pass of their own
        fz.profile(True)
        for _ in range(3):
            fn()
        fz.synchronize()
        st = fz.profile_read()
        fz.profile(False)
        res["merge"][name]["stage_ms"] = {k: round(v[0] / 3, 4) for k, v in st.items() if v[2]}
        res["merge"][name]["stage_launches"] = {k: v[2] // 3 for k, v in st.items() if v[2]}
        print(f"  {name:<44} {res['merge'][name]}", flush=True)
    return res


def value(sky, huber):
    lay = PL.config_layout("C1")
    out_w, ew = PL.CONFIGS["C1"]
    oh = out_w // 2
    fz = panofuse.Fuser(0)
    fz.set_tiles(lay)
    seeds = pf_synth.seeds_for(1)
    emap = pf_synth.baseline_emap(seeds, ew, ew // 2, device=DEV).contiguous()
    clean, gt = disparity_tiles(fz, lay, seeds, out_w)
    # every tile pixel's zenith as a fraction of pi: the equirectangular row ramp, warped as the
    # scene is (no tone response)
    ramp = ((torch.arange(oh, device=DEV, dtype=torch.float32) + 0.5) / oh)[None, :, None]
    ramp = ramp.expand(1, oh, out_w).contiguous()
    zen = torch.zeros((1, fz.tile_elems), dtype=torch.float32, device=DEV)
    fz.warp_depth(ramp, zen, None)
    fz.synchronize()
    skyd = torch.where(zen < sky, torch.zeros_like(clean), clean).contiguous()
    nlevels = panofuse.level_info(out_w, oh, ZR, 0)[5]
    _, _, h0, h1, _, _ = panofuse.level_info(out_w, oh, ZR, nlevels - 1)
    gtn = gt[0].cpu().numpy().astype(np.float64)
    first = max(h0, int(np.ceil(sky * oh)))

    def band_error(out):
        err = np.abs(out.cpu().numpy().view(np.uint16)[0].astype(np.float64) / 65535.0 - gtn)
        return {"band_error": float(err[h0:h1 + 1].mean()),
                "band_error_below_sky": float(err[first:h1 + 1].mean())}

    res = {"sky_zenith_fraction": sky, "huber_a": huber,
           "sky_share_of_tile_pixels": float((zen < sky).float().mean())}

    def run(name, tiles, how):
        out = torch.zeros((1, oh, out_w), dtype=torch.int16, device=DEV)
        cf = torch.zeros((1, lay.ntiles, 4), dtype=torch.float32, device=DEV)
        if how == "range":
            w = fz.range_weights(tiles, 0.0, INF)
            fz.merge_disparity_weighted(emap, tiles, w, out, ZR, coeffs=cf)
        else:
            if how == "huber":
                fz.set_register_loss("huber", huber)
            try:
                fz.merge_disparity(emap, tiles, out, ZR, coeffs=cf)
            finally:
                fz.set_register_loss(None)
        fz.synchronize()
        res[name] = band_error(out)
        res[name]["coeffs"] = cf.cpu().numpy()[0].tolist()
        print(f"  {name:<28} band error {res[name]['band_error']:.5f}  below the sky line "
              f"{res[name]['band_error_below_sky']:.5f}", flush=True)

    print(f"value: C1, sky above zenith {sky} pi "
          f"({100 * res['sky_share_of_tile_pixels']:.1f} % of the tile pixels)")
    run("sky tiles, unweighted", skyd, "plain")
    run("sky tiles, range:0:inf", skyd, "range")
    run(f"sky tiles, huber {huber}", skyd, "huber")
    run("clean tiles, unweighted", clean, "plain")
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("parts", nargs="*", default=["cost", "value"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--sky", type=float, default=0.40)
    ap.add_argument("--huber", type=float, default=0.05)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("disp_weights_value needs a GPU: nothing is measured without one")
    result = {}
    if "value" in a.parts:
        result["value"] = value(a.sky, a.huber)
    if "cost" in a.parts:
        print("cost: C3")
        result["cost"] = cost(a.runs, a.warmup, a.inner)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
