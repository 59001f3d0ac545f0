"""Times pf_layout_audit (k_layout_audit: the counter reset, the kernel, the 48-byte read-back)
per level with device events: median of --runs calls after --warmup warm-ups, the level caches
built beforehand.  Prints one JSON line per (layout, output width).

Usage (on the GPU): python tools/audit_probe.py [--runs 9] [--warmup 2]"""
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
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch

    import panofuse
    import pf_layouts as PL
    if not torch.cuda.is_available():
        sys.exit("audit_probe needs a GPU")
    zr = PL.ZENITH_RANGE
    fz = panofuse.Fuser(0)
    for name, lay, out_w in (("leres", PL.leres_layout(), 2048), ("midas", PL.midas_layout(), 2048),
                             ("C5", PL.config_layout("C5"), 8192)):
        fz.set_tiles(lay)
        nlev = panofuse.level_info(out_w, out_w // 2, zr, 0)[5]
        first = [fz.layout_audit(out_w, zr, lv) for lv in range(nlev)]  # builds the level caches
        times = [[] for _ in range(nlev)]
        for i in range(a.warmup + a.runs):
            for lv in range(nlev):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(fz.stream)
                fz.layout_audit(out_w, zr, lv)
                e1.record(fz.stream)
                e1.synchronize()
                if i >= a.warmup:
                    times[lv].append(e0.elapsed_time(e1))
        print(json.dumps({
            "layout": name, "ntiles": lay.ntiles, "out_w": out_w, "runs": a.runs,
            "levels": [[r["w"], r["h"]] for r in first],
            "audit_ms": [round(statistics.median(t), 4) for t in times],
            "audit_ms_min": [round(min(t), 4) for t in times],
            "audit_ms_max": [round(max(t), 4) for t in times],
            "last_level": first[-1]}))


if __name__ == "__main__":
    main()
