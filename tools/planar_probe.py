"""Time the planar-depth tile path (pf_set_tile_depth) against the ray-distance path at the C3
shape: 64 panoramas, 20 tiles of 512^2 (2,409 samples per tile), a 512 x 256 baseline, a 2048 x 1024
output.  The figures are pf_profile_read's stages (hipEvent pairs around each stage) over `steps`
calls, per call, for `runs` runs, RAY against PLANAR:

  register/moment, register/huber, register/disparity   the register stage with apply off
  apply        the register stage with apply on minus the one with apply off (moment form)
  merge        the sum of all stages of pf_merge; under PLANAR its register stage holds the
               apply-into-copy pass

The tiles are the synthetic warp divided by the ray factor, so the planar fits work on what a
perspective network would give.  It reports, it is no yardstick: no threshold is set.

Usage (on the GPU): python tools/planar_probe.py [--batch 64] [--runs 3] [--steps 10] [--warmup 2]
                                                  [--layout C3|C1]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wacv2023-high-resolution-depth-estimation-for-panoramas-"
                                      "through-perspective-map-registrations_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--layout", choices=("C3", "C1"), default="C3")
    a = ap.parse_args()
    import torch

    import panofuse
    import pf_layouts as PL
    import pf_synth
    if not torch.cuda.is_available():
        sys.exit("planar_probe needs a GPU")
    dev = torch.device("cuda:0")
    zr = PL.ZENITH_RANGE
    lay = PL.config_layout(a.layout)
    out_w, ew = (2048, 512) if a.layout == "C3" else (512, 128)
    B, nt = a.batch, lay.ntiles
    fz = panofuse.Fuser(0)
    fz.set_tiles(lay)
    seeds = pf_synth.seeds_for(B)
    emap = pf_synth.baseline_emap(seeds, ew, ew // 2, device=dev).contiguous()
    gt = pf_synth.scene_depth(seeds, out_w, out_w // 2, device=dev).contiguous()
    tiles = torch.zeros((B, fz.tile_elems), dtype=torch.float32, device=dev)
    fz.warp_depth(gt, tiles, panofuse.make_responses(pf_synth.responses(seeds, nt), dev))
    kf = fz.tile_ray_factor()
    fz.synchronize()
    tiles = (tiles / kf[None, :]).contiguous()
    inv = 1.0 / tiles.clamp_min(0.02)
    disp = ((inv - inv.amin(1, keepdim=True))
            / (inv.amax(1, keepdim=True) - inv.amin(1, keepdim=True))).contiguous()
    work = torch.empty_like(tiles)
    cf = torch.zeros((B, nt, 4), dtype=torch.float32, device=dev)
    out = torch.zeros((B, out_w // 2, out_w), dtype=torch.int16, device=dev)

    def timed(call, pick):
        for _ in range(a.warmup):
            call()
        fz.synchronize()
        res = []
        for _ in range(a.runs):
            fz.profile(True)
            for _ in range(a.steps):
                call()
            fz.synchronize()
            res.append(round(pick(fz.profile_read()) / a.steps, 5))
            fz.profile(False)
        return res

    def reg(p):
        return p["register"][0]

    def whole(p):
        return sum(v[0] for v in p.values())

    def apply_call():
        work.copy_(tiles)  # outside the library's stages: not timed
        fz.register(emap, work, zr, degree=3, apply=True, coeffs=cf)

    res = {"layout": a.layout, "shape": {"batch": B, "tiles": nt, "kf_max": float(kf.max())},
           "runs": a.runs, "steps": a.steps, "ms": {}}
    for depth in ("ray", "planar"):
        fz.set_tile_depth(depth)
        m = {}
        m["register/moment"] = timed(
            lambda: fz.register(emap, tiles, zr, degree=3, apply=False, coeffs=cf), reg)
        fz.set_register_loss("huber", 0.02)
        m["register/huber"] = timed(
            lambda: fz.register(emap, tiles, zr, degree=3, apply=False, coeffs=cf), reg)
        fz.set_register_loss(None)
        m["register/disparity"] = timed(
            lambda: fz.register_disparity(emap, disp, zr, apply=False, coeffs=cf), reg)
        with_apply = timed(apply_call, reg)
        m["register+apply/moment"] = with_apply
        m["apply"] = [round(x - y, 5) for x, y in zip(with_apply, m["register/moment"])]
        m["merge"] = timed(lambda: fz.merge(emap, tiles, out, zr, coeffs=cf), whole)
        m["merge register stage"] = timed(lambda: fz.merge(emap, tiles, out, zr, coeffs=cf), reg)
        res["ms"][depth] = m
    fz.set_tile_depth("ray")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
