"""Time the direct stitch and the Laplacian self-check (csrc/pf_stitch.hip) at the C3 shape.

* Fuser.stitch on --batch panoramas of 2048 x 1024 from 20 tiles of 512^2 with coefficients, the
  map cached (the first call builds it; its one-off time is reported apart).  Algorithmic bytes:
  2 B per output pixel + 4 B per covered pixel (the tile value); the 8 B per pixel of the cached
  map come on top and are served from cache after the first panorama.  The fraction of the HBM peak
  (8.0 TB/s) printed is that algorithmic figure over the measured time.
* Fuser.laplacian_residual on one 2048 x 1024 plane and on --batch planes (rows of the C3 band).
* Fuser.solve_smoothing at the same shape, whole call (its seed and quantise stages are two of its
  kernels: see --kernel-stats).

Device events around --inner back-to-back calls; medians of --runs windows after --warmup
warm-ups, per call.  No threshold is set: nothing existed to compare against.

--trace: a short sequence (1 cold + 3 warm stitches, 1 smoothing, 1 residual per size) for a
  kernel trace, as
  rocprofv3 --kernel-trace --stats -d DIR -o run --output-format csv -- python tools/stitch_probe.py --trace
--kernel-stats CSV: adds the average times of k_stitch and of the smoothing's k_smooth_seed and
  k_quantize (its seed-plus-quantise stages: 4 B gathered + 4 B written, then 4 B read + 2 B
  written per pixel) from that run's kernel stats to the JSON.

Writes one JSON line to stdout and to profiles/stitch/stitch_probe.json.

Usage (on the GPU): python tools/stitch_probe.py [--batch 64] [--runs 7] [--warmup 2] [--inner 10]"""
import argparse
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wacv2023-high-resolution-depth-estimation-for-panoramas-"
                                      "through-perspective-map-registrations_amd"))
HBM_PEAK = 8.0e12  # bytes per second
W, H = 2048, 1024


def kernel_stats(path):
    """{kernel: (calls, average ms)} of the stitch and the smoothing's seed / quantise kernels."""
    out = {}
    with open(path) as f:
        rows = csv.DictReader(ln for ln in f if not ln.startswith("#"))
        for r in rows:
            for k in ("k_stitch_map", "k_stitch", "k_smooth_seed", "k_quantize", "k_lap_residual"):
                name = r["Name"].split("(")[0]
                if name.endswith("::" + k) or name == k:
                    out[k] = {"calls": int(r["Calls"]), "avg_ms": float(r["AverageNs"]) * 1e-6,
                              "min_ms": float(r["MinNs"]) * 1e-6}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stitch", "stitch_probe.json"))
    a = ap.parse_args()
    if a.runs < 5 or a.warmup < 2:
        sys.exit("stitch_probe: at least 2 warm-ups and 5 runs")
    import torch

    import panofuse
    import pf_layouts as PL
    if not torch.cuda.is_available():
        sys.exit("stitch_probe needs a GPU")
    dev = torch.device("cuda:0")
    zr = PL.ZENITH_RANGE
    B = a.batch
    lay = PL.config_layout("C3")
    fz = panofuse.Fuser(0)
    fz.set_tiles(lay)
    g = torch.Generator(device=dev).manual_seed(20261020)
    tiles = torch.rand((B, fz.tile_elems), generator=g, dtype=torch.float32, device=dev)
    cf = torch.tensor([0.1, -0.2, 1.05, 0.01], dtype=torch.float32, device=dev)
    cf = cf.repeat(B, lay.ntiles, 1).contiguous()
    out = torch.zeros((B, H, W), dtype=torch.int16, device=dev)
    _, _, h0, h1, _, _ = panofuse.level_info(W, H, zr, 2)
    planes = torch.rand((B, H, W), generator=g, dtype=torch.float32, device=dev)
    lnorm = (torch.rand((B, H, W), generator=g, dtype=torch.float32, device=dev) - 0.5) * 0.1
    err = torch.zeros(B, dtype=torch.float32, device=dev)

    def timed(fn, n=1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(fz.stream)
        for _ in range(n):
            fn()
        e1.record(fz.stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    def stitch():
        fz.stitch(tiles, out, coeffs=cf)

    def smoothing():
        fz.solve_smoothing(tiles, out, zr, coeffs=cf)

    def residual_1():
        fz.laplacian_residual(planes[:1], lnorm[:1], h0, h1, err=err[:1])

    def residual_b():
        fz.laplacian_residual(planes, lnorm, h0, h1, err=err)

    first_ms = timed(stitch)  # builds and caches the map
    if a.trace:  # every k_stitch / k_smooth_seed / k_quantize dispatch is one of the whole batch
        for _ in range(3):
            stitch()
        smoothing()
        residual_1()
        residual_b()
        fz.synchronize()
        print(json.dumps({"trace": True, "batch": B}))
        return
    # covered pixels: ones through the identity cubic quantise to 65535, no tile gives 0
    ones = torch.ones((1, fz.tile_elems), dtype=torch.float32, device=dev)
    fz.stitch(ones, out[:1])
    fz.synchronize()
    covered = int((out[0] != 0).sum())
    calls = (("stitch", stitch, a.inner), ("laplacian_residual_1", residual_1, 1),
             (f"laplacian_residual_{B}", residual_b, 1), ("solve_smoothing", smoothing, 1))
    times = {name: [] for name, _, _ in calls}
    for i in range(a.warmup + a.runs):
        for name, fn, n in calls:
            ms = timed(fn, n)
            if i >= a.warmup:
                times[name].append(ms)
    npx = W * H
    stitch_bytes = B * (2.0 * npx + 4.0 * covered)
    res = {"shape": {"batch": B, "output": [W, H], "layout": lay.name, "tiles": lay.ntiles,
                     "covered_pixels": covered, "band_rows": [h0, h1]},
           "runs": a.runs, "warmup": a.warmup, "inner_calls_stitch": a.inner,
           "hbm_peak_tbs": HBM_PEAK / 1e12, "stitch_first_call_ms": round(first_ms, 4)}
    for name, _, _ in calls:
        ms = statistics.median(times[name])
        res[name] = {"ms": round(ms, 5), "ms_min": round(min(times[name]), 5),
                     "ms_max": round(max(times[name]), 5)}
    ms = res["stitch"]["ms"]
    res["stitch"].update({"algorithmic_bytes": stitch_bytes,
                          "algorithmic_tbs": round(stitch_bytes / (ms * 1e-3) / 1e12, 4),
                          "algorithmic_hbm_peak_fraction":
                              round(stitch_bytes / (ms * 1e-3) / HBM_PEAK, 4)})
    terms = (h1 - h0 - 1) * (W - 2)
    for name in ("laplacian_residual_1", f"laplacian_residual_{B}"):
        res[name]["terms_per_plane"] = terms
        res[name]["ns_per_term"] = round(res[name]["ms"] * 1e6 / terms, 3)
    if a.kernel_stats:
        ks = kernel_stats(a.kernel_stats)
        res["kernel_stats"] = {k: {"calls": v["calls"], "avg_ms": round(v["avg_ms"], 5),
                                   "min_ms": round(v["min_ms"], 5)} for k, v in ks.items()}
        if "k_smooth_seed" in ks and "k_quantize" in ks:
            sq = ks["k_smooth_seed"]["avg_ms"] + ks["k_quantize"]["avg_ms"]
            res["kernel_stats"]["smoothing_seed_plus_quantize_ms"] = round(sq, 5)
            res["kernel_stats"]["smoothing_seed_plus_quantize_bytes"] = B * 10.0 * npx
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
