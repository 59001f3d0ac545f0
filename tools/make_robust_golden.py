"""Regenerate tests/golden/robust_ref.npz: registration sample arrays with what real Ceres 1.13
(the reference's vendored tree, DENSE_SCHUR, default options) returns for them under
ceres::HuberLoss(a) and ceres::SoftLOneLoss(a).

tools/robust_ref_harness.cpp is compiled in a temporary directory with build_harness(with_ceres=
True) of tools/make_global_golden.py's kind (tools/make_edge_golden.py); nothing built is kept.

Cases (CASES): the six "scene" tiles of tests/fusion_ref.py's c1_256x128 with 10 % of the sampled
baseline values (y) replaced by U(0, 1) and clamped; tile 0 clean; tile 0 as a disparity tile
(per-tile normalised inverse depth) with the same planting.  Recorded per case k: xs{k}, ys{k}
(float64, clamped, as fed to Ceres) and model{k}; per case x loss x scale (LOSSES x SCALES), in
that order: coef [n][4], cost [n][2] (initial, final), entries [n] (the length of
Summary::iterations), type [n] (Summary::termination_type) and message [n].

For every record the tool prints the restatement's (tests/robust_ref.py) iteration count,
termination and largest fitted-value difference at the samples.

Usage (where the reference tree exists): python tools/make_robust_golden.py REFERENCE_DIR"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "tools", "oracle",
          "wacv2023-high-resolution-depth-estimation-for-panoramas-through-perspective-map-"
          "registrations_amd"):
    sys.path.insert(0, os.path.join(ROOT, p))
import disp_ref as DR  # noqa: E402
import fusion_ref as FR  # noqa: E402
import pyoracle as O  # noqa: E402
import robust_ref as R  # noqa: E402
from make_edge_golden import build_harness  # noqa: E402

LOSSES = ("huber", "softl1")
SCALES = (0.02, 0.005)
# (tile, model, planted)
CASES = [(p, "cubic", True) for p in range(6)] + [(0, "cubic", False), (0, "disparity", True)]
OUT = os.path.join(ROOT, "tests", "golden", "robust_ref.npz")


def case_samples(golden, k):
    tile, model, planted = CASES[k]
    _, tiles, data, emap, _, zr = FR.case_inputs(golden, "c1_256x128")
    if model == "disparity":
        t = tiles[tile]
        n = t.width * t.height
        data = data.copy()
        inv = np.float32(1.0) / np.maximum(data[t.offset:t.offset + n], np.float32(0.02))
        data[t.offset:t.offset + n] = (inv - inv.min()) / (inv.max() - inv.min())
    xs, ys, _, _ = O.reg_samples(tiles[tile], data, emap, zr)
    if planted:
        rng = np.random.default_rng(3100 + k)
        hit = rng.random(ys.size) < 0.10
        ys = ys.copy()
        ys[hit] = rng.uniform(0, 1, int(hit.sum()))
        ys = DR.clamp_samples(ys)
    return xs, ys, model


def main():
    if len(sys.argv) != 2 or not os.path.exists(os.path.join(sys.argv[1], "Depth.cpp")):
        sys.exit("usage: make_robust_golden.py REFERENCE_DIR (the tree that holds Depth.cpp)")
    ref = os.path.abspath(sys.argv[1])
    golden = np.load(os.path.join(ROOT, "tests", "golden", "fusion_ref.npz"))
    out = {"losses": np.array(LOSSES), "scales": np.array(SCALES, np.float64)}
    coef, cost, entries, types, msgs = [], [], [], [], []
    with tempfile.TemporaryDirectory() as d:
        exe = build_harness(ref, d, os.path.join(ROOT, "tools", "robust_ref_harness.cpp"),
                            with_ceres=True)
        for k in range(len(CASES)):
            xs, ys, model = case_samples(golden, k)
            out[f"xs{k}"], out[f"ys{k}"], out[f"model{k}"] = xs, ys, np.array(model)
            xf, yf = os.path.join(d, "xs.f64"), os.path.join(d, "ys.f64")
            xs.tofile(xf)
            ys.tofile(yf)
            for loss in LOSSES:
                for a in SCALES:
                    r = subprocess.run([exe, model, loss, repr(a), str(xs.size), xf, yf],
                                       check=True, capture_output=True, text=True)
                    rows = {ln.split(" ", 1)[0]: ln.split(" ", 1)[1]
                            for ln in r.stdout.splitlines() if " " in ln}
                    c = np.array([float(v) for v in rows["FIT"].split()], np.float64)
                    coef.append(c)
                    cost.append([float(v) for v in rows["COST"].split()])
                    entries.append(int(rows["ITER"]))
                    types.append(int(rows["TYPE"]))
                    msgs.append(rows["MSG"])
                    mine, s = R.fit(xs, ys, loss, a, model)
                    if model == "cubic":
                        dv = np.max(np.abs(R.cubic(mine, xs) - R.cubic(c, xs)))
                    else:
                        dv = np.max(np.abs(1.0 / (mine[0] * xs + mine[1]) + mine[3]
                                           - (1.0 / (c[0] * xs + c[1]) + c[3])))
                    print(f"case {k} {CASES[k]} {loss} a={a}: ceres {entries[-1]} entries, "
                          f"'{msgs[-1]}', cost {cost[-1][0]:.9g} -> {cost[-1][1]:.9g}; "
                          f"restatement {s['iterations']} iterations, {s['termination']}, "
                          f"cost {s['initial_cost']:.9g} -> {s['final_cost']:.9g}; "
                          f"max |fit diff| at the samples {dv:.3g}", flush=True)
    out["coef"] = np.array(coef, np.float64)
    out["cost"] = np.array(cost, np.float64)
    out["entries"] = np.array(entries, np.int32)
    out["type"] = np.array(types, np.int32)
    out["message"] = np.array(msgs)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
