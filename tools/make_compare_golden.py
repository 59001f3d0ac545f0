"""Regenerate tests/golden/compare_ref.npz: small map pairs as image files with what the
reference's own DepthNamespace::ErrorCompare (Depth.cpp:2460-2634) returns for them -- its seven
floats and the shifted 8-bit PNG it writes.

The reference's unmodified Depth.cpp is compiled in a temporary directory with
tools/compare_ref_harness.cpp the way tools/make_edge_golden.py does it (build_harness); nothing
built here is kept.

Nine input pairs: gt 64x32 / given 64x32, 100x50 / 64x33 and 75x37 / 75x37 as 16-bit PNGs; the
baseline also as a mono360 "Pf" PFM, an RGB8 and a gray+alpha 8-bit PNG; the gt also as RGB8.
Each runs in depth mode and in disparity mode with several align_way / cap settings (RUNS).  The
gt has 15 % black pixels and reaches 1.0; the baseline is 0.03 / gt + 0.3 + noise, zero where the
gt is zero, so the disparity fit has o < 0, the masked pixels turn black and a few pixels reach
the cap of 10.

Recorded: the distinct raw arrays (array_names, array_kinds: index into compare_ref.KINDS),
pairs [npairs][2] (gt array, given array), runs [nruns][4] (pair, disp, align_way, cap), ref
[nruns][7] float32 (parsed from %.9g), plane_of [npairs][2] (the plane of a pair in depth and
in disparity mode: the plane ignores align_way / cap, and pairs that share a baseline share their
depth-mode plane), pixels{j} and png{j} per plane (the reference's shifted plane as stbi_load
returns it and the file's bytes), and save8_plane / save8_png: the 8-bit plane of the 5x3 map
(float)i * 0.1f - 0.25f (values below 0 and above 1) and the reference's PNG of that plane
(stbi_write_png, one channel, through a depth-mode run on an 8-bit baseline that quantises to
it), which EquirectangularMap::Save8bit must reproduce.

Usage (where the reference tree exists): python tools/make_compare_golden.py REFERENCE_DIR"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "oracle", "tools",
          "wacv2023-high-resolution-depth-estimation-for-panoramas-through-perspective-map-"
          "registrations_amd"):
    sys.path.insert(0, os.path.join(ROOT, p))
import compare_ref as R  # noqa: E402
import pf_layouts as PL  # noqa: E402
from make_edge_golden import build_harness  # noqa: E402

# (disp, align_way, cap) per pair
RUNS = [(0, 1, 1), (0, 0, 0), (1, 0, 1), (1, 1, 1), (1, 2, 0), (1, 1, 0)]
# (gt array, given array): names of ARRAYS
PAIRS = [("gt16_a", "giv16_a"), ("gt16_b", "giv16_b"), ("gt16_c", "giv16_c"),
         ("gt16_a", "givpfm_a"), ("gt16_a", "givrgb_a"), ("gt16_a", "givga_a"),
         ("gtrgb_a", "giv16_a"), ("gtrgb_c", "givpfm_c"), ("gt16_b", "givga_b")]


def scene(h, w):
    y, x = np.mgrid[0:h, 0:w]
    u, v = x / w, y / h
    s = 0.5 + 0.3 * np.sin(6.3 * u + 1.0) * np.cos(3.1 * v) + 0.15 * (u > 0.4) - 0.1 * (v > 0.6)
    return np.clip(s, 0.08, 1.0)


def make_arrays(rng):
    """The distinct raw arrays by name, with their file kind."""
    out = {}
    shapes = {"a": ((32, 64), (32, 64)), "b": ((50, 100), (33, 64)), "c": ((37, 75), (37, 75))}
    for tag, ((gh, gw), (h, w)) in shapes.items():
        g = scene(gh, gw)
        black = rng.random((gh, gw)) < 0.15
        # 11-bit steps: the low bits of a smooth 16-bit map only cost bytes in the fixture
        g16 = (np.clip(g * 2047.0, 1, 2047).astype(np.uint16) * 32).astype(np.uint16)
        g16[g >= 1.0] = 65535
        g16[black] = 0
        out[f"gt16_{tag}"] = (g16, "png16")
        g8 = np.zeros((gh, gw, 3), np.uint8)
        g8[..., 0] = np.clip(g * 255.0 + 0.5, 1, 255).astype(np.uint8)
        g8[..., 0][black] = 0
        g8[..., 1] = 7
        g8[..., 2] = np.arange(gh, dtype=np.uint8)[:, None]
        out[f"gtrgb_{tag}"] = (g8, "png8")
        # the baseline at its own size: a disparity of the scene, zero where the gt pixel that
        # the reference pairs with it is zero
        ys = (np.arange(h, dtype=np.float32) * (np.float32(gh) / np.float32(h))).astype(int)
        xs = (np.arange(w, dtype=np.float32) * (np.float32(gw) / np.float32(w))).astype(int)
        d = 0.03 / scene(h, w) + 0.3 + rng.normal(0, 0.001, (h, w))
        # 48 pixels around the disparity that the fit maps to zero (about 0.29): their s * v + o
        # is negative (black) or small (a depth above the cap of 10)
        spots = rng.choice(h * w, 48, replace=False)
        d.reshape(-1)[spots] = np.linspace(0.280, 0.300, 48)
        d[black[np.ix_(ys, xs)]] = 0.0
        d = np.clip(d, 0.0, 1.0)
        out[f"giv16_{tag}"] = ((np.round(d * 8191.0) * 8).astype(np.uint16), "png16")
        # bottom-up rows, as a PFM stores them: the mono360 load flips them back
        out[f"givpfm_{tag}"] = ((np.round(d * 8192.0) / 8192.0 * 8.0).astype(np.float32)[::-1].copy(),
                                "pfm")
        d8 = (d * 255.0 + 0.5).astype(np.uint8)
        rgb = np.zeros((h, w, 3), np.uint8)
        rgb[..., 0], rgb[..., 1] = d8, 200
        rgb[..., 2] = np.arange(w, dtype=np.uint8)[None, :]
        out[f"givrgb_{tag}"] = (rgb, "png8")
        ga = np.zeros((h, w, 2), np.uint8)
        ga[..., 0], ga[..., 1] = d8, 255
        out[f"givga_{tag}"] = (ga, "png8")
    return out


def run(exe, d, gt, gt_kind, given, given_kind, disp, align, cap):
    gfn = os.path.join(d, "gt" + R.extension(gt_kind))
    vfn = os.path.join(d, "given" + R.extension(given_kind))
    sfn = os.path.join(d, "shifted.png")
    R.write_file(gfn, gt, gt_kind)
    R.write_file(vfn, given, given_kind)
    r = subprocess.run([exe, gfn, vfn, str(disp), str(align), str(cap), sfn], check=True,
                       capture_output=True, text=True)
    cmp_line = [ln for ln in r.stdout.splitlines() if ln.startswith("CMP ")][0]
    pix_line = [ln for ln in r.stdout.splitlines() if ln.startswith("PIX ")][0].split()
    w, h, c = (int(t) for t in pix_line[1:4])
    assert c == 1
    pixels = np.frombuffer(bytes.fromhex(pix_line[4]), np.uint8).reshape(h, w)
    ref = np.array([np.float32(t) for t in cmp_line.split()[1:]], np.float32)
    return ref, pixels, np.frombuffer(open(sfn, "rb").read(), np.uint8)


def save8_map():
    """The 5x3 map that tests/cpp/compare_link.cpp fills by hand: (float)i * 0.1f - 0.25f, from
    -0.25 to 1.15, so Save8bit clamps at both ends."""
    i = np.arange(15, dtype=np.float32)
    return ((i * np.float32(0.1)).astype(np.float32) - np.float32(0.25)).astype(np.float32).reshape(3, 5)


def save8_input():
    """An 8-bit given map whose depth-mode shifted plane is Save8bit's plane of save8_map()."""
    want = R.save8bit(save8_map())
    assert want.min() == 0 and want.max() == 255 and (want == 0).sum() >= 2 and (want == 255).sum() >= 2
    src = want.copy()
    for _ in range(2):  # (u8 / 255.0f) * 255.0f may land just below the integer
        low = R.quantise(R.load_map(src, "png8")) < want
        src[low] += 1
    assert np.array_equal(R.quantise(R.load_map(src, "png8")), want)
    return src, want


def main():
    if len(sys.argv) != 2 or not os.path.exists(os.path.join(sys.argv[1], "Depth.cpp")):
        sys.exit("usage: make_compare_golden.py REFERENCE_DIR (the tree that holds Depth.cpp)")
    ref_dir = os.path.abspath(sys.argv[1])
    rng = np.random.default_rng(20261019)
    arrays = make_arrays(rng)
    used = []
    for g, v in PAIRS:
        for n in (g, v):
            if n not in used:
                used.append(n)
    out = {"array_names": np.array(used), "array_kinds":
           np.array([R.KINDS.index(arrays[n][1]) for n in used], np.int32),
           "pairs": np.array([[used.index(g), used.index(v)] for g, v in PAIRS], np.int32)}
    for n in used:
        out[n] = arrays[n][0]
    runs, refs, planes = [], [], []
    plane_of = [[-1, -1] for _ in PAIRS]
    worst = 0
    with tempfile.TemporaryDirectory() as d:
        exe = build_harness(ref_dir, d, os.path.join(ROOT, "tools", "compare_ref_harness.cpp"))
        for k, (gn, vn) in enumerate(PAIRS):
            (g, gk), (v, vk) = arrays[gn], arrays[vn]
            for disp, align, cap in RUNS:
                ref, pixels, png = run(exe, d, g, gk, v, vk, disp, align, cap)
                mine = R.compare(R.load_map(g, gk), R.load_map(v, vk, True), PL.ZENITH_RANGE,
                                 disp, align, cap)
                mf = np.array([mine[m] for m in R.METRICS], np.float32)
                same = bool(np.array_equal(mf.view(np.uint32), ref.view(np.uint32)))
                npx = int((mine["shifted"] != pixels).sum())
                worst += (not same) + npx
                if plane_of[k][disp] >= 0:  # the plane ignores align_way / cap
                    assert png.tobytes() == planes[plane_of[k][disp]][1].tobytes()
                else:
                    same_png = [j for j, pl in enumerate(planes) if pl[1].tobytes() == png.tobytes()]
                    if not same_png:
                        planes.append((pixels, png))
                    plane_of[k][disp] = same_png[0] if same_png else len(planes) - 1
                runs.append((k, disp, align, cap))
                refs.append(ref)
                extra = ""
                if disp:
                    dp = mine["depth"]
                    extra = (f" fit ({mine['fit_s']:.6g}, {mine['fit_o']:.6g}) black "
                             f"{dp.size - mine['n_nonblack']}/{dp.size} at cap {(dp == 10).sum()}")
                print(f"pair {k} ({gn}, {vn}) disp {disp} align {align} cap {cap}: metrics equal "
                      f"{same}, {npx} pixels differ{extra}")
        src, want = save8_input()
        gt5 = np.full((3, 5), 30000, np.uint16)
        _, pixels, png = run(exe, d, gt5, "png16", src, "png8", 0, 0, 0)
        assert np.array_equal(pixels, want)
        out["save8_plane"], out["save8_png"] = want, png
    out["runs"] = np.array(runs, np.int32)
    out["plane_of"] = np.array(plane_of, np.int32)
    for j, (pixels, png) in enumerate(planes):
        out[f"pixels{j}"], out[f"png{j}"] = pixels, png
    out["ref"] = np.stack(refs)
    dst = os.path.join(ROOT, "tests", "golden", "compare_ref.npz")
    np.savez_compressed(dst, **out)
    print(dst, os.path.getsize(dst), "bytes,", len(out), "arrays,", len(runs), "runs;",
          "restatement mismatches:", worst)


if __name__ == "__main__":
    main()
