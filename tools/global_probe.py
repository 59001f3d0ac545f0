"""Time the post-fusion calibration kernels (csrc/pf_global.hip) at the C3 shape:
Fuser.register_global with apply (the global cubic fit of SolveDepthToDepth2 and the u16
transform) on --batch panoramas of 2048 x 1024 over 512 x 256 baselines, its fit and its transform
alone, and Fuser.median_scale on --batch float maps of 2048 x 1024 toward maps of the same size.
Device events around --inner back-to-back calls; the medians of --runs windows after --warmup
warm-ups, per call.  No threshold is set: nothing existed to compare against.

Each entry carries its algorithmic bytes and the fraction of the HBM peak (8.0 TB/s; a float4
copy reaches 6.29 TB/s on this part) they amount to at the measured time:
  fit        the band's u16 read once (2 B per sample) + one baseline float per sample read from
             a 512 x 256 map that stays in cache: counted once per panorama
  transform  the band's u16 read and written (4 B per sample)
  median     three histogram passes over both maps (channel 0, 4 B per pixel) + the scaling pass
             over map 0 (read and write)

The result planes are the baselines upsampled, drifted by a cubic and quantised, so the fit has
something to find; the kernels' times do not depend on the values (the LM runs on 15 sums).
Writes one JSON line to stdout and to profiles/global/global_probe.json.

Usage (on the GPU): python tools/global_probe.py [--batch 64] [--runs 9] [--warmup 2] [--inner 10]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wacv2023-high-resolution-depth-estimation-for-panoramas-"
                                      "through-perspective-map-registrations_amd"))
HBM_PEAK = 8.0e12  # bytes per second


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "global", "global_probe.json"))
    a = ap.parse_args()
    import torch

    import panofuse
    import pf_layouts as PL
    import pf_synth
    if not torch.cuda.is_available():
        sys.exit("global_probe needs a GPU")
    dev = torch.device("cuda:0")
    zr = PL.ZENITH_RANGE
    W, H, ew, eh = 2048, 1024, 512, 256
    B = a.batch
    fz = panofuse.Fuser(0)
    seeds = pf_synth.seeds_for(B)
    emap = pf_synth.baseline_emap(seeds, ew, eh, device=dev).contiguous()
    gt = pf_synth.scene_depth(seeds, W, H, device=dev).contiguous()
    drift = (0.8 * gt.clamp(0, 1) ** 1.3 + 0.06).clamp(0, 1)
    q = (drift * 65535.0).to(torch.int32)
    src = torch.where(q >= 32768, q - 65536, q).to(torch.int16).contiguous()  # u16 bits
    data = src.clone()
    cf = torch.zeros((B, 4), dtype=torch.float32, device=dev)
    sm = torch.zeros((B, 4), dtype=torch.float64, device=dev)
    map0 = gt.clamp(0, 1).contiguous()
    map1 = (drift * 0.7).contiguous()
    work0 = map0.clone()
    med = torch.zeros((B, 2), dtype=torch.float32, device=dev)
    st = torch.zeros((B,), dtype=torch.int32, device=dev)
    _, _, h0, h1, _, _ = panofuse.level_info(W, H, zr, 2)
    ns = W * (h1 - h0 + 1)

    def fit_apply():
        fz.register_global(emap, data, zr, apply=True, coeffs=cf, summary=sm)

    def fit():
        fz.register_global(emap, data, zr, apply=False, coeffs=cf, summary=sm)

    def transform():
        fz.result_transform(data, zr, cf)

    def median():
        fz.median_scale(work0, map1, medians=med, status=st)

    calls = (("register_global_apply", fit_apply), ("register_global_fit", fit),
             ("result_transform", transform), ("median_scale", median))
    times = {name: [] for name, _ in calls}
    for i in range(a.warmup + a.runs):
        for name, fn in calls:
            # every window starts from the same planes (the transform and the scaling work in
            # place); the copies are outside the events
            data.copy_(src)
            work0.copy_(map0)
            if name == "result_transform":
                fit()  # its coefficients
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(fz.stream)
            for _ in range(a.inner):
                fn()
            e1.record(fz.stream)
            e1.synchronize()
            if i >= a.warmup:
                times[name].append(e0.elapsed_time(e1) / a.inner)
    data.copy_(src)
    fit()
    fz.synchronize()
    s = sm.cpu().numpy()
    fit_bytes = B * (2.0 * ns + 4.0 * ew * eh)
    tr_bytes = B * 4.0 * ns
    med_bytes = B * (3 * 2 * 4.0 * W * H + 8.0 * W * H)
    bytes_of = {"register_global_apply": fit_bytes + tr_bytes, "register_global_fit": fit_bytes,
                "result_transform": tr_bytes, "median_scale": med_bytes}
    res = {"shape": {"batch": B, "result": [W, H], "baseline": [ew, eh], "band_rows": [h0, h1],
                     "samples": ns, "chunks": (ns + 16383) // 16384},
           "runs": a.runs, "inner_calls": a.inner, "hbm_peak_tbs": HBM_PEAK / 1e12,
           "lm_iterations": {"min": int(s[:, 2].min()), "max": int(s[:, 2].max())},
           "terminations": {str(int(k)): int((s[:, 3] == k).sum()) for k in sorted(set(s[:, 3]))}}
    for name, _ in calls:
        ms = statistics.median(times[name])
        res[name] = {"ms": round(ms, 5), "ms_min": round(min(times[name]), 5),
                     "ms_max": round(max(times[name]), 5), "bytes": bytes_of[name],
                     "tbs": round(bytes_of[name] / (ms * 1e-3) / 1e12, 4),
                     "hbm_peak_fraction": round(bytes_of[name] / (ms * 1e-3) / HBM_PEAK, 4)}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
