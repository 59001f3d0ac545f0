"""Time the disparity registration (Fuser.register_disparity: the sample-wise LM fit of
y = 1/(a x + b) + d, csrc/pf_disp.hip) against the cubic registration (Fuser.register: the
moment-form LM of k_register) at the C3 shape: --batch panoramas x the 20 tiles of the C2 layout
(512^2 tiles, 73 x 33 = 2409 samples each), a 512 x 256 baseline (--layout C1: 6 tiles of 256^2,
7865 samples each, a 128 x 64 baseline).  Both are timed in the same
process on the same buffers, alternating, with device events around --inner back-to-back calls;
the medians of --runs windows after --warmup warm-ups, per call.  The cubic registration is the
yardstick: no threshold is set.  Also prints the fit's iteration counts and termination codes
(its per-tile summary) so a time can be read against the work done.  Prints one JSON line.

Where the time goes: a block's time is its LM iterations times the cost of one, and the call ends
with its slowest block.  The probe therefore also times one panorama alone (20 blocks on 20 CUs:
the time of the slowest block) for the panorama holding the tile with the most iterations and for
the one whose slowest tile has the fewest; the two points give the cost per iteration and the
fixed cost.  --layout C1 repeats everything at 7865 samples per tile (31 per lane instead of 10):
the change of the per-iteration cost is the share of the sample passes, the rest is the ten-sum
reductions and the serial LM algebra every lane repeats.

The tiles are per-tile normalised inverse depth of the synthetic depth tiles (MiDaS' convention);
the cubic registration reads the same buffers (its time does not depend on the values).

Usage (on the GPU): python tools/disp_probe.py [--batch 64] [--runs 9] [--warmup 2] [--inner 20]
                                                [--layout C3|C1]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wacv2023-high-resolution-depth-estimation-for-panoramas-"
                                      "through-perspective-map-registrations_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--layout", choices=("C3", "C1"), default="C3")
    a = ap.parse_args()
    import torch

    import panofuse
    import pf_layouts as PL
    import pf_synth
    if not torch.cuda.is_available():
        sys.exit("disp_probe needs a GPU")
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
    depth = torch.zeros((B, fz.tile_elems), dtype=torch.float32, device=dev)
    resp = panofuse.make_responses(pf_synth.responses(seeds, nt), dev)
    fz.warp_depth(gt, depth, resp)
    fz.synchronize()
    per = depth.view(B, nt, -1)
    inv = 1.0 / per.clamp(min=0.02)
    lo, hi = inv.amin(dim=2, keepdim=True), inv.amax(dim=2, keepdim=True)
    tiles = ((inv - lo) / (hi - lo)).reshape(B, -1).contiguous()
    cf = torch.zeros((B, nt, 4), dtype=torch.float32, device=dev)
    sm = torch.zeros((B, nt, 4), dtype=torch.float64, device=dev)

    def disparity():
        fz.register_disparity(emap, tiles, zr, apply=False, coeffs=cf, summary=sm)

    def cubic():
        fz.register(emap, tiles, zr, degree=3, apply=False, coeffs=cf)

    calls = (("register_disparity", disparity), ("register_cubic", cubic))
    times = {name: [] for name, _ in calls}
    for i in range(a.warmup + a.runs):
        for name, fn in calls:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(fz.stream)
            for _ in range(a.inner):
                fn()
            e1.record(fz.stream)
            e1.synchronize()
            if i >= a.warmup:
                times[name].append(e0.elapsed_time(e1) / a.inner)
    disparity()
    fz.synchronize()
    s = sm.cpu().numpy().reshape(-1, 4)
    its = s[:, 2].astype(int)
    med = {k: statistics.median(v) for k, v in times.items()}

    def one_panorama(b):  # per-call ms of register_disparity on panorama b alone
        e1m, t1 = emap[b:b + 1], tiles[b:b + 1]
        c1 = torch.zeros((1, nt, 4), dtype=torch.float32, device=dev)
        t = []
        for i in range(a.warmup + a.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(fz.stream)
            for _ in range(a.inner):
                fz.register_disparity(e1m, t1, zr, apply=False, coeffs=c1)
            e1.record(fz.stream)
            e1.synchronize()
            if i >= a.warmup:
                t.append(e0.elapsed_time(e1) / a.inner)
        return statistics.median(t)

    worst = its.reshape(B, nt).max(axis=1)  # each panorama's slowest tile
    b_hi, b_lo = int(worst.argmax()), int(worst.argmin())
    t_hi, t_lo = one_panorama(b_hi), one_panorama(b_lo)
    it_hi, it_lo = int(worst[b_hi]), int(worst[b_lo])
    per_it = (t_hi - t_lo) / (it_hi - it_lo) if it_hi > it_lo else float("nan")
    print(json.dumps({
        "layout": a.layout, "shape": {"batch": B, "tiles": nt}, "runs": a.runs,
        "inner_calls": a.inner,
        "register_disparity_ms": round(med["register_disparity"], 5),
        "register_disparity_ms_min": round(min(times["register_disparity"]), 5),
        "register_disparity_ms_max": round(max(times["register_disparity"]), 5),
        "register_cubic_ms": round(med["register_cubic"], 5),
        "register_cubic_ms_min": round(min(times["register_cubic"]), 5),
        "register_cubic_ms_max": round(max(times["register_cubic"]), 5),
        "ratio": round(med["register_disparity"] / med["register_cubic"], 3),
        "lm_iterations": {"min": int(its.min()), "median": float(statistics.median(its.tolist())),
                          "max": int(its.max())},
        "terminations": {str(int(k)): int((s[:, 3] == k).sum()) for k in sorted(set(s[:, 3]))},
        "final_over_initial_cost_max": float((s[:, 1] / s[:, 0]).max()),
        "one_panorama": {"most_iterations": it_hi, "ms": round(t_hi, 5),
                         "fewest_iterations": it_lo, "ms_fewest": round(t_lo, 5),
                         "us_per_iteration": round(per_it * 1e3, 3),
                         "fixed_us": round((t_lo - per_it * it_lo) * 1e3, 3)}}))


if __name__ == "__main__":
    main()
