"""Time pf_error_compare (Fuser.compare_async) in disparity mode at 64 x 2048 x 1024 float against
a float gt of the same size, tree order, with device events: median of --runs calls after --warmup
warm-ups.  The floor the composite cannot beat -- its two pf_error_metrics calls alone (align_way 2
uncapped on the gt's disparity, then align_way 1 capped on the depth plane) -- is timed in the same
process on the same buffers, alternating with it.  The difference is what the new kernels cost;
it is set against their algorithmic bytes at the stream ceiling this project has measured
(5.1-5.25 TB/s, profiles/r03/stream_mix.txt): 4 read + 4 written per gt pixel (the gt's disparity
plane), 4 * given_c read + 4 written per given pixel (the fused pass), 4 read + 1 written (the
quantise pass).  Prints one JSON line.

Usage (on the GPU): python tools/compare_probe.py [--batch 64] [--runs 9] [--warmup 2]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "wacv2023-high-resolution-depth-estimation-for-panoramas-"
                                      "through-perspective-map-registrations_amd"))
STREAM_CEILING = 5.1e12  # bytes/s, the lower end of the measured range


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch

    import panofuse
    import pf_layouts as PL
    if not torch.cuda.is_available():
        sys.exit("compare_probe needs a GPU")
    dev = "cuda:0"
    B, w, h = a.batch, a.width, a.width // 2
    g = torch.Generator(device=dev).manual_seed(20261019)
    gt = torch.rand((B, h, w), generator=g, device=dev) * 0.9 + 0.08
    black = torch.rand((B, h, w), generator=g, device=dev) < 0.15
    gt[black] = 0.0
    given = 0.03 / gt.clamp(min=0.05) + 0.3 + 0.003 * torch.randn((B, h, w), generator=g, device=dev)
    given[black] = 0.0
    given = given.contiguous()
    fz = panofuse.Fuser(0)
    fz.set_metrics_order("tree")
    out_c = torch.zeros((B, panofuse.COMPARE_WORDS), dtype=torch.int32, device=dev)
    out_m = torch.zeros((B, 16), dtype=torch.int32, device=dev)
    depth = torch.empty((B, h, w), dtype=torch.float32, device=dev)
    shifted = torch.empty((B, h, w), dtype=torch.uint8, device=dev)
    # the floor's inputs: the planes the composite itself makes
    fz.compare_async(gt, given, PL.ZENITH_RANGE, out_c, True, 1, True, depth, shifted)
    gt_disp = gt.clone()
    fz.disp_depth_convert(gt_disp)
    fz.synchronize()
    depth_in = depth.clone()

    def compare():
        fz.compare_async(gt, given, PL.ZENITH_RANGE, out_c, True, 1, True, depth, shifted)

    def compare_noplanes():
        fz.compare_async(gt, given, PL.ZENITH_RANGE, out_c, True, 1, True, None, shifted)

    def metrics2():
        fz.error_metrics_async(gt_disp, given, PL.ZENITH_RANGE, out_m, 2, False)
        fz.error_metrics_async(gt, depth_in, PL.ZENITH_RANGE, out_m, 1, True)

    conv_buf = gt.clone()

    def conv():  # the gt pass alone, in place: the same 4 read + 4 written per pixel
        fz.disp_depth_convert(conv_buf)

    calls = (("compare", compare), ("compare_scratch_depth", compare_noplanes),
             ("metrics2", metrics2), ("conv", conv))
    times = {name: [] for name, _ in calls}
    for i in range(a.warmup + a.runs):
        for name, fn in calls:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(fz.stream)
            fn()
            e1.record(fz.stream)
            e1.synchronize()
            if i >= a.warmup:
                times[name].append(e0.elapsed_time(e1))
    med = {k: statistics.median(v) for k, v in times.items()}
    npx = B * w * h
    nbytes = npx * (8 + 8 + 5)
    extra_ms = med["compare"] - med["metrics2"]
    first = fz.compare(gt[:1], given[:1], PL.ZENITH_RANGE, True, 1, True)[0]
    print(json.dumps({
        "shape": [B, h, w], "runs": a.runs,
        "compare_ms": round(med["compare"], 4), "compare_ms_min": round(min(times["compare"]), 4),
        "compare_ms_max": round(max(times["compare"]), 4),
        "compare_scratch_depth_ms": round(med["compare_scratch_depth"], 4),
        "metrics2_ms": round(med["metrics2"], 4), "conv_pass_ms": round(med["conv"], 4),
        "conv_pass_bytes_per_s": round(npx * 8 / (med["conv"] * 1e-3), 0),
        "new_kernels_ms": round(extra_ms, 4), "new_kernels_bytes": nbytes,
        "new_kernels_bytes_per_s": round(nbytes / (extra_ms * 1e-3), 0),
        "share_of_stream_ceiling": round(nbytes / (extra_ms * 1e-3) / STREAM_CEILING, 4),
        "fit_first": [first["fit_s"], first["fit_o"]], "minmax_first": [first["vmin"], first["vmax"]],
        "n_nonblack_first": first["n_nonblack"], "mae_first": first["mae"]}))


if __name__ == "__main__":
    main()
