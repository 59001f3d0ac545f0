"""Regenerate tests/golden/fusion_ref.npz: what the compiled reference returns from
SolveDepthToDepth (real Ceres 1.13), Depth2DepthTransform, SolveDepthAll, SolveDepthBySmoothing
and ErrorData for the cases of tests/fusion_ref.py.

The reference's unmodified Depth.cpp is compiled in a temporary directory with
tools/fusion_ref_harness.cpp and the vendored Ceres the way tools/make_global_golden.py does it
(build_harness(with_ceres=True), about a minute).  The harness builds the maps in memory and calls
the reference's functions only; nothing built here is kept.

Every case runs twice, under OMP_NUM_THREADS=1 and 4: SolveDepthAll accumulates overlapping
tiles inside `#pragma omp critical` in the order the threads arrive.  If the two runs differ in
one output bit or in the number of "[SolveDepthAll] oops!" lines, the tool refuses to write the
fixture.  It also refuses a case whose levels do not double, where the oracle counts a tap index
outside its tile (the reference reads out of bounds there), or where the reference's "oops!"
lines and the oracle's count differ.

Recorded (see tests/fusion_ref.py for the case table and the sha256 + subsample form):
  tiles_<set> uint8, base* / gt uint16        the inputs
  <case>_abcd float32 [n][4]                   SolveDepthToDepth, one tile active at a time
  <case>_tiles uint32 bits                     the tiles after Depth2DepthTransform
  <case>_out uint16 [H][W]                     SolveDepthAll / SolveDepthBySmoothing
  <case>_metrics uint32 [6][8]                 ErrorData per (align_way, cap_depth)
  <case>_oops int64                            the reference's "oops!" lines
  joint<k>_abcd float32 [4]                    SolveDepthToDepth over JOINT_SETS[k]

Per case the tool prints how the oracle (oracle/pf_oracle.c) compares, and at the end the number
of disagreements and the largest ulp distance of a coefficient.

Usage (where the reference tree exists):
    python tools/make_fusion_golden.py REFERENCE_DIR [BUILT_HARNESS]
BUILT_HARNESS: an executable of the harness built earlier by this tool's recipe; skips the
build."""
import io
import os
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "tools", "oracle",
          "wacv2023-high-resolution-depth-estimation-for-panoramas-through-perspective-map-"
          "registrations_amd"):
    sys.path.insert(0, os.path.join(ROOT, p))
import fusion_ref as F  # noqa: E402
import pyoracle as O  # noqa: E402
from make_edge_golden import build_harness  # noqa: E402

PANO = (512, 256)


def scene(h, w):
    """A smooth panorama with two depth edges, values in 0.08 .. 0.92."""
    y, x = np.mgrid[0:h, 0:w]
    u, v = x / w, y / h
    s = 0.5 + 0.22 * np.sin(6.2832 * u + 1.0) * np.cos(3.1 * v) + 0.12 * np.sin(12.5664 * u) \
        + 0.1 * (v > 0.55) - 0.08 * ((u > 0.3) & (u < 0.45))
    return np.clip(s, 0.08, 0.92)


def detail(h, w):
    """Five periods around and three down: every 72-degree window sees the whole value range."""
    y, x = np.mgrid[0:h, 0:w]
    u, v = x / w, y / h
    return 0.5 + 0.42 * np.sin(6.2832 * 5 * u + 0.7) * np.sin(6.2832 * 3 * v + 0.3)


def make_tiles(lay, rng, stretch=1.0, scene=scene):
    """The scene warped into the layout's tiles by the oracle's E->P gather (inputs only: the
    fixture stores the tiles themselves), a per-tile response, noise, 8 bits."""
    tiles, total = O.make_tiles(lay)
    pano = scene(PANO[1], PANO[0]).astype(np.float32)
    t = O.warp_depth(pano, tiles, total, None).astype(np.float64)
    out = np.zeros(total, np.uint8)
    for p, tl in enumerate(tiles):
        n = tl.width * tl.height
        v = t[tl.offset:tl.offset + n]
        v = (0.85 - 0.03 * p) * v ** (1.15 + 0.05 * (p % 3)) + 0.04 + 0.01 * p
        v = (v - 0.5) * stretch + 0.5
        out[tl.offset:tl.offset + n] = np.clip(np.round(v * 255.0) + rng.integers(-3, 4, n), 0, 255)
    return out.reshape(lay.ntiles, int(lay.tile_h[0]), int(lay.tile_w[0]))


def make_inputs():
    rng = np.random.default_rng(20261020)
    inp = {}
    c1 = F.layout("C1", (64, 64))
    inp["tiles_scene"] = make_tiles(c1, rng)
    inp["tiles_leres_narrow"] = make_tiles(F.layout("LERES", (48, 40)), rng)
    inp["tiles_leres"] = make_tiles(F.layout("LERES", (48, 40)), rng, scene=detail)
    inp["tiles_wide"] = make_tiles(F.layout("WIDE", (64, 64)), rng)
    # clamps: stretched so that whole regions saturate, plus patches of exact 0 and 255 in every
    # tile: the 1e-4 / 1 - 1e-4 sample clamps and both clamps of Depth2DepthTransform fire
    t = make_tiles(c1, rng, stretch=2.6)
    t[:, :12, :20] = 0
    t[:, -14:, -18:] = 255
    t[:, 28:36, :] = np.where(np.arange(64)[None, None, :] % 16 < 8, 0, 255)
    inp["tiles_clamps"] = t
    d = make_tiles(c1, rng)
    d[0] = 128                                              # constant
    d[1] = np.where(rng.random((64, 64)) < 0.5, 64, 192)    # two-valued
    d[2] = 0                                                # all zero
    # only 0 and 1, as two regions: with two x values only a + b + c and d are determined, and a
    # salt-and-pepper mask gives both values the same mean baseline, so a + b + c vanishes and a
    # relative bar on a, b, c would measure rounding noise over ~0 (measured on such a tile:
    # 2e-8 absolute in both LM forms, which is 1e-4 relative to a = 2.2e-4)
    yy, xx = np.mgrid[0:64, 0:64]
    d[3] = np.where(xx + yy < 64, 0, 255)
    d[4, :, :32] = 0                                        # half zero
    inp["tiles_degenerate"] = d
    for name, (ew, eh, ec) in F.BASELINES.items():
        b = (detail if name == "base40d" else scene)(eh, ew) * 0.9 + 0.03 \
            + rng.normal(0, 0.004, (eh, ew))
        if name == "base40c":  # saturated at both ends: the baseline sample clamps fire, and the
            b = (b - 0.5) * 8.0 + 0.5  # fitted cubic leaves 0..1, so the transform's clamps do
        b16 = np.clip(np.round(b * 65535.0), 0, 65535).astype(np.uint16)
        if ec > 1:  # Value reads channel 0 only: the others must not matter
            m = np.zeros((eh, ew, ec), np.uint16)
            m[..., 0] = b16
            m[..., 1] = 16384
            m[..., 2] = (np.arange(ew) * 65535 // ew).astype(np.uint16)[None, :]
            b16 = m
        inp[name] = b16
    gh, gw = F.GT_SHAPE
    g = np.clip(np.round(scene(gh, gw) * 0.35 * 65535.0), 7, 65535).astype(np.uint16)
    g[20:27, 30:44] = 0  # a zero patch inside the band
    g[rng.random((gh, gw)) < 0.02] = 0
    inp["gt"] = g
    return inp


def write_case(fn, lay, data, emap, size, zr, gt, active=None):
    n = lay.ntiles
    ew, eh, ec = (emap.shape[1], emap.shape[0], emap.shape[2] if emap.ndim == 3 else 1)
    gw, gh = (gt.shape[1], gt.shape[0]) if gt is not None else (0, 0)
    act = np.zeros(n, np.int32)
    if active is not None:
        act[list(active)] = 1
    with open(fn, "wb") as f:
        f.write(np.array([n, lay.tile_w[0], lay.tile_h[0], ew, eh, ec, size[0], size[1], gw, gh],
                         np.int32).tobytes())
        f.write(np.array(zr, np.float32).tobytes())
        f.write(act.tobytes())
        f.write(np.concatenate([lay.fovs, lay.ranges], 1).astype(np.float32).tobytes())
        f.write(np.ascontiguousarray(data, np.float32).tobytes())
        f.write(np.ascontiguousarray(emap, np.float32).tobytes())
        if gt is not None:
            f.write(np.ascontiguousarray(gt, np.float32).tobytes())


def run_both(exe, mode, cfn, ofn):
    """The harness under 1 and 4 threads: (output bytes, oops lines), or exits if they differ."""
    res = []
    for threads in ("1", "4"):
        env = dict(os.environ, OMP_NUM_THREADS=threads)
        r = subprocess.run([exe, mode, cfn, ofn], check=True, capture_output=True, text=True,
                           env=env)
        # counted as a substring: the threads' unlocked std::cout writes can share one line
        oops = r.stdout.count("[SolveDepthAll] oops!")
        res.append((open(ofn, "rb").read(), oops))
    if res[0] != res[1]:
        a, b = (np.frombuffer(r[0], np.uint8) for r in res)
        sys.exit(f"{mode} {cfn}: the 1-thread and 4-thread runs differ ({int((a != b).sum())} "
                 f"bytes, oops {res[0][1]} / {res[1][1]}): the reference is indeterminate here; "
                 "not writing the fixture")
    return res[0]


def save_npz(path, arrays):
    """np.savez_compressed with a fixed member date, so that a rerun is byte-identical."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            a = np.asarray(arrays[name])
            np.lib.format.write_array(buf, a if a.ndim == 0 else np.ascontiguousarray(a),
                                      allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main():
    if len(sys.argv) not in (2, 3) or not os.path.exists(os.path.join(sys.argv[1], "Depth.cpp")):
        sys.exit("usage: make_fusion_golden.py REFERENCE_DIR [BUILT_HARNESS]")
    ref_dir = os.path.abspath(sys.argv[1])
    out = make_inputs()
    gt = F.map_f32(out["gt"])
    bad = 0
    worst_ulp = {"moments": 0, "samples": 0}
    any_oops = 0
    with tempfile.TemporaryDirectory() as d:
        exe = sys.argv[2] if len(sys.argv) == 3 else build_harness(
            ref_dir, d, os.path.join(ROOT, "tools", "fusion_ref_harness.cpp"), with_ceres=True)
        cfn, ofn = os.path.join(d, "case.bin"), os.path.join(d, "out.bin")
        for case, (mode, lname, tile, tset, (W, H), base, zr) in F.CASES.items():
            lay, tiles, data, emap, _, _ = F.case_inputs(out, case)
            n, tn = lay.ntiles, data.size
            whole = case in F.WHOLE
            if not F.levels_double(W, H, zr):
                sys.exit(f"{case}: the levels of {W}x{H} do not double")
            stub = emap if emap is not None else np.zeros((2, 2), np.float32)
            write_case(cfn, lay, data, stub, (W, H), zr, gt if mode == "merge" else None)
            raw, oops = run_both(exe, mode, cfn, ofn)
            msg = []
            if mode == "merge":
                abcd = np.frombuffer(raw, np.float32, n * 4).reshape(n, 4).copy()
                tt = np.frombuffer(raw, np.float32, tn, n * 16).copy()
                res = np.frombuffer(raw, np.uint16, W * H, n * 16 + tn * 4).reshape(H, W).copy()
                met = np.frombuffer(raw, np.uint32, 48, n * 16 + tn * 4 + W * H * 2)
                met = met.reshape(6, 8).copy()
                out[case + "_abcd"] = abcd
                F.record_plane(out, case + "_tiles", F.bits(tt).reshape(n, tile[1], tile[0]), whole)
                out[case + "_metrics"] = met
                kap = F.tile_kappas(tiles, data, emap, zr)
                ill = tuple(p for p, k in enumerate(kap) if k > F.KAPPA_MAX)
                if case not in F.SPLIT and ill != F.ILL_CONDITIONED.get(case, ()):
                    sys.exit(f"{case}: ill-conditioned tiles {ill}, kappa " +
                             " ".join(f"{k:.2g}" for k in kap))
                msg.append(f"kappa {min(kap):.2g}..{max(kap):.2g}")
                for form in ("moments", "samples"):
                    a, dt = F.oracle_register(tiles, data, emap, zr, form)
                    ulp = int(F.ulp_diff(a, abcd).max())
                    worst_ulp[form] = max(worst_ulp[form], ulp)
                    abad = F.abcd_mismatch(a, abcd, kap, case in F.SPLIT)
                    if case in F.SPLIT:  # transform and fusion from the recorded coefficients
                        own = int((F.bits(dt) != F.bits(tt)).sum())
                        dt = data.copy()
                        for p in range(n):
                            O.depth_to_depth(tiles[p], dt, abcd[p])
                    tbad = int((F.bits(dt) != F.bits(tt)).sum())
                    o, _ = O.solve_depth_all(emap, tiles, dt, W, zr, out_h=H)
                    obad = int((o != res).sum())
                    bad += tbad + obad + len(abad)
                    rel = float(F.rel_diff(a, abcd).max())
                    msg.append(f"{form}: abcd {ulp} ulp (rel {rel:.2g}, missing its bar: "
                               f"{abad}), tiles {tbad}, u16 {obad}" +
                               (f" (from its own coefficients: tiles {own})"
                                if case in F.SPLIT else ""))
                o_oops, oob = F.oracle_levels(tiles, tt, W, H, zr)
                mbad = 0
                for k, (aw, cap) in enumerate(F.SETTINGS):
                    # ErrorData reads the global g_zenith_range (Depth.cpp:22, 1983), not the
                    # range the fusion was given
                    m = F.metric_bits(O.error_metrics(gt, res, F.ZR, aw, bool(cap)), aw)
                    mbad += int((m != met[k]).sum())
                bad += mbad
                msg.append(f"ErrorData words differing {mbad}")
            else:
                res = np.frombuffer(raw, np.uint16, W * H).reshape(H, W).copy()
                if mode == "fuse":
                    o, _ = O.solve_depth_all(emap, tiles, data, W, zr, out_h=H)
                    o_oops, oob = F.oracle_levels(tiles, data, W, H, zr)
                else:
                    o = O.solve_smoothing(tiles, data, W, H, zr)
                    o_oops = 0  # SolveDepthBySmoothing prints nothing
                    _, _, _, oob = O.targets(tiles, data, O.Level(W, H, 0, H - 1, 1, 3))
                obad = int((o != res).sum())
                bad += obad
                msg.append(f"u16 {obad}")
            if oob:
                sys.exit(f"{case}: the oracle counts {oob} tap indices outside their tile")
            if oops != o_oops:
                sys.exit(f"{case}: the reference printed {oops} oops lines, the oracle counts "
                         f"{o_oops}")
            any_oops += oops
            F.record_plane(out, case + "_out", res, whole)
            out[case + "_oops"] = np.int64(oops)
            print(f"{case}: {mode} {W}x{H} nonzero {int((res != 0).sum())} oops {oops} (oracle "
                  f"{o_oops}, oob {oob}); oracle vs reference: " + "; ".join(msg), flush=True)
        lay, tiles, data, emap, _, zr = F.case_inputs(out, "c1_256x128")
        for k, active in enumerate(F.JOINT_SETS):
            write_case(cfn, lay, data, emap, (8, 8), zr, None, active)
            raw, _ = run_both(exe, "joint", cfn, ofn)
            abcd = np.frombuffer(raw, np.float32, 4).copy()
            out[f"joint{k}_abcd"] = abcd
            xs, ys = F.joint_samples(tiles, data, emap, zr, active)
            c, s = O.lm_fit(xs, ys)
            ulp = int(F.ulp_diff(c.astype(np.float32), abcd).max())
            rel = float(F.rel_diff(c.astype(np.float32), abcd).max())
            worst_ulp["samples"] = max(worst_ulp["samples"], ulp)
            bad += rel > 1e-5
            print(f"joint {active}: {xs.size} samples, abcd {abcd.tolist()}; oracle's sample-wise "
                  f"LM {ulp} ulp (rel {rel:.2g}, {s['iterations']} iterations, "
                  f"{s['termination']})", flush=True)
    if not any_oops:
        sys.exit("no case has an oops line: the count comparison is vacuous")
    dst = os.path.join(ROOT, "tests", "golden", "fusion_ref.npz")
    save_npz(dst, out)
    print(dst, os.path.getsize(dst), "bytes,", len(out), "arrays; disagreements:", int(bad),
          "; largest coefficient distance, ulp: moment form", worst_ulp["moments"],
          "sample-wise", worst_ulp["samples"])


if __name__ == "__main__":
    main()
