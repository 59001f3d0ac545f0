"""Regenerate tests/golden/edge_metrics_ref.npz: small 16-bit PNG pairs with the five doubles the
reference's own DepthNamespace::ErrorLaplacian (Depth.cpp:2636-2953) returns for them.

The reference's unmodified Depth.cpp is compiled in a temporary directory with
tools/edge_ref_harness.cpp, without building Ceres: ErrorLaplacian needs only Load and ValueAtXY,
so the objects are split per function (-ffunction-sections -fdata-sections) and the linker drops
everything the harness does not reach (-Wl,--gc-sections), the solver calls included.  The Ceres
config.h comes from a configure-only cmake run of the vendored tree; windows.h and
opencv2/opencv.hpp are two shim headers.  Nothing built here is kept.

Recorded per pair k: gt{k} / given{k} (u16 [h][w]), ref{k} (the reference's lap_mse, lap_mae,
sobelx_mae, sobely_mae, lap5_mae, parsed from %.17g) and counts{k} (n_lap, n_sobel, n_lap5 of
the restatement tests/edge_ref.py: the reference does not print its counts).

Usage (where the reference tree exists): python tools/make_edge_golden.py REFERENCE_DIR"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import edge_ref as E  # noqa: E402

# (gt h, gt w), (given h, given w): equal, gt larger (integer ratio), gt larger (non-integer),
# gt smaller, equal with odd sizes
PAIRS = [((32, 64), (32, 64)), ((64, 128), (32, 64)), ((50, 100), (33, 64)),
         ((33, 64), (50, 100)), ((37, 75), (37, 75))]

WINDOWS_H = """#pragma once
typedef unsigned long DWORD;
static inline DWORD timeGetTime() { return 0; }
"""
OPENCV_HPP = """#pragma once
#define CV_16UC1 2
namespace cv {
struct Mat {
    int rows, cols, type; void* data;
    Mat(int r, int c, int t, void* d) : rows(r), cols(c), type(t), data(d) {}
};
static inline bool imwrite(const char*, const Mat&) { return false; }
}
"""


def make_pair(rng, gshape, vshape):
    """A smooth scene with edges plus noise; the given map is the scene blurred and offset.
    About 3 % of the gt pixels are zero and its top rows form a zero band."""
    def scene(h, w):
        y, x = np.mgrid[0:h, 0:w]
        u, v = x / w, y / h
        s = 0.35 + 0.2 * np.sin(6.3 * u + 1.0) * np.cos(3.1 * v) + 0.15 * (u > 0.4) - 0.1 * (v > 0.6)
        return s
    gh, gw = gshape
    h, w = vshape
    g = scene(gh, gw) + rng.normal(0, 0.01, (gh, gw))
    v = scene(h, w) * 0.97 + 0.01 + rng.normal(0, 0.02, (h, w))
    g16 = np.clip(g * 65535.0, 7, 65535).astype(np.uint16)
    v16 = np.clip(v * 65535.0, 0, 65535).astype(np.uint16)
    g16[rng.random((gh, gw)) < 0.03] = 0
    g16[:max(2, gh // 10)] = 0
    return g16, v16


def build_harness(ref, d, harness=None, with_ceres=False):
    """Compile the reference's Depth.cpp with a harness (tools/edge_ref_harness.cpp unless another
    path is given) into d; returns the executable.  with_ceres: also build the configured Ceres
    tree (ninja, at most 16 jobs; about a minute) and link its archive, for a harness that
    reaches the solver calls."""
    harness = harness or os.path.join(ROOT, "tools", "edge_ref_harness.cpp")
    shim = os.path.join(d, "shim")
    os.makedirs(os.path.join(shim, "opencv2"))
    open(os.path.join(shim, "windows.h"), "w").write(WINDOWS_H)
    open(os.path.join(shim, "opencv2", "opencv.hpp"), "w").write(OPENCV_HPP)
    ceres = os.path.join(d, "ceres")
    subprocess.run(["cmake", "-S", os.path.join(ref, "ceres-solver"), "-B", ceres, "-G", "Ninja",
                    "-DCMAKE_BUILD_TYPE=Release", "-DCMAKE_POLICY_VERSION_MINIMUM=3.5",
                    "-DEIGEN_INCLUDE_DIR=" + os.path.join(ref, "eigen"), "-DCXSPARSE=OFF",
                    "-DLAPACK=OFF", "-DSUITESPARSE=OFF", "-DMINIGLOG=ON", "-DGFLAGS=OFF",
                    "-DBUILD_TESTING=OFF"] +
                   (["-DCMAKE_CXX_FLAGS=-DERROR=ERROR_ -w"] if with_ceres else []),
                   check=True, stdout=subprocess.DEVNULL)
    libs = []
    if with_ceres:
        jobs = str(min(16, os.cpu_count() or 1))
        subprocess.run(["ninja", "-C", ceres, "-j", jobs], check=True, stdout=subprocess.DEVNULL)
        libs = sorted(os.path.join(ceres, "lib", f) for f in os.listdir(os.path.join(ceres, "lib"))
                      if f.endswith(".a"))
    exe = os.path.join(d, os.path.splitext(os.path.basename(harness))[0])
    inc = [shim, ref, os.path.join(ref, "ilmbase22", "include"),
           os.path.join(ref, "ceres-solver", "include"), os.path.join(ceres, "config"),
           os.path.join(ref, "ceres-solver", "internal", "ceres", "miniglog"),
           os.path.join(ref, "eigen")]
    subprocess.run(["g++", "-std=c++14", "-O2", "-fopenmp", "-w", "-DERROR=ERROR_",
                    "-ffunction-sections", "-fdata-sections"] + ["-I" + i for i in inc] +
                   [harness, os.path.join(ref, "Depth.cpp")] + libs +
                   ["-Wl,--gc-sections", "-o", exe],
                   check=True)
    return exe


def main():
    if len(sys.argv) != 2 or not os.path.exists(os.path.join(sys.argv[1], "Depth.cpp")):
        sys.exit("usage: make_edge_golden.py REFERENCE_DIR (the tree that holds Depth.cpp)")
    ref = os.path.abspath(sys.argv[1])
    rng = np.random.default_rng(20261019)
    out = {}
    with tempfile.TemporaryDirectory() as d:
        exe = build_harness(ref, d)
        for k, (gs, vs) in enumerate(PAIRS):
            g16, v16 = make_pair(rng, gs, vs)
            gfn, vfn = os.path.join(d, "gt.png"), os.path.join(d, "given.png")
            E.write_png16(gfn, g16)
            E.write_png16(vfn, v16)
            r = subprocess.run([exe, gfn, vfn], check=True, capture_output=True, text=True)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("EDGE ")][0]
            vals = np.array([float(t) for t in line.split()[1:]], np.float64)
            mine = E.edge_metrics(E.u16_to_float(g16), E.u16_to_float(v16))
            out[f"gt{k}"], out[f"given{k}"], out[f"ref{k}"] = g16, v16, vals
            out[f"counts{k}"] = np.array([mine[c] for c in E.COUNTS], np.int64)
            h, w = vs
            worst = max(abs(mine[key] - vals[i]) / abs(vals[i]) for i, key in enumerate(E.KEYS))
            print(f"pair {k}: gt {gs} given {vs} counts {out[f'counts{k}'].tolist()} "
                  f"restatement vs reference: worst rel {worst:.3g} (bound {E.mean_bound(w, h):.3g})")
            print("   ", r.stdout.strip().splitlines()[0])
    dst = os.path.join(ROOT, "tests", "golden", "edge_metrics_ref.npz")
    np.savez_compressed(dst, **out)
    print(dst, os.path.getsize(dst), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
