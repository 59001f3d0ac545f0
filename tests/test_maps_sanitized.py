"""The facade's host-only maps unit under AddressSanitizer + UBSan -- CPU only.

csrc/pf_depth_maps.cpp (the map classes' loads, accessors and moves, Metrics::Save, the PNG
writers) includes neither HIP nor panofuse.h, so the host compiler builds it with pf_image.cpp and
pf_jpeg.cpp.  tests/cpp/maps_check.cpp (its own main) links them with
-fsanitize=address,undefined -fno-sanitize-recover=all and loads a directory of small files --
8- and 16-bit PNG (gray and RGB), a PGM, a PFM, a baseline JPEG, each of them also cut at half
its length, and an empty file -- into both map classes, twice, reads, saves and moves the maps.
It runs as a child process; nothing sanitized is loaded into Python.  Every line it prints must
equal the unsanitized library's pfd_load_map on the same file (dimensions and a hash of the float
bits), so the sanitized run took the same paths; the four LoadPfm variants are held to numpy."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

import panofuse
from codec_cases import png_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.dirname(os.path.dirname(panofuse.LIB_PATH))


def _fnv(a):
    h = 1469598103934665603
    for b in np.ascontiguousarray(a, np.float32).tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def _files(d, L):
    rng = np.random.default_rng(11)
    w, h = 7, 5
    files = {"gray8.png": png_bytes(rng.integers(0, 256, (h, w, 1)), 8, 0),
             "gray16.png": png_bytes(rng.integers(0, 65536, (h, w, 1)), 16, 0, seed=1),
             "rgb8.png": png_bytes(rng.integers(0, 256, (h, w, 3)), 8, 2, seed=2),
             "rgb16.png": png_bytes(rng.integers(0, 65536, (h, w, 3)), 16, 2, seed=3),
             "gray.pgm": b"P5\n7 5\n255\n" + rng.integers(0, 256, (h, w), dtype=np.uint8).tobytes()}
    pfm = rng.normal(3, 8, (h, w)).astype(np.float32)
    files["depth.pfm"] = b"Pf\n7 5\n-1.0\n" + pfm.astype("<f4").tobytes()
    px = rng.integers(0, 256, (16, 24, 3), dtype=np.uint8)
    jpg = d / "rgb.jpg"
    assert L.pfd_save_jpeg(os.fsencode(jpg), px.ctypes.data, 24, 16, 3, 90, 0) == 0
    files["rgb.jpg"] = jpg.read_bytes()
    for name, data in list(files.items()):
        stem, ext = name.rsplit(".", 1)
        files[f"{stem}_half.{ext}"] = data[:len(data) // 2]
    files["empty.png"] = b""
    for name, data in files.items():
        (d / name).write_bytes(data)
    return sorted(files), pfm


def test_maps_unit_under_asan_ubsan(tmp_path):
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    assert cxx is not None, "no host C++ compiler"
    exe = tmp_path / "maps_check"
    csrc = os.path.join(PKG, "csrc")
    # no ROCm include path: the three units are host code
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                        os.path.join(ROOT, "tests", "cpp", "maps_check.cpp"),
                        os.path.join(csrc, "pf_depth_maps.cpp"), os.path.join(csrc, "pf_image.cpp"),
                        os.path.join(csrc, "pf_jpeg.cpp"), "-lz", "-o", str(exe)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]

    L = C.CDLL(os.path.join(PKG, "lib", "libpanofuse_depth.so"))
    ip = C.POINTER(C.c_int)
    L.pfd_load_map.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_longlong, ip, ip, ip]
    L.pfd_save_jpeg.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                C.c_int]
    d, out = tmp_path / "files", tmp_path / "out"
    d.mkdir()
    out.mkdir()
    names, pfm = _files(d, L)

    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1")
    r = subprocess.run([str(exe), str(d), str(out)], capture_output=True, text=True, timeout=300,
                       env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "maps_check ok" in r.stdout
    got = {tuple(ln.split()[:2]): ln.split()[2:] for ln in r.stdout.splitlines()
           if ln[:1] in "EPF" and len(ln.split()) == 7}

    loaded = 0
    for name in names:
        for tag, is_emap in (("E", 1), ("P", 0)):
            w, h, c = C.c_int(), C.c_int(), C.c_int()
            buf = np.zeros(4096, np.float32)
            rc = L.pfd_load_map(os.fsencode(d / name), is_emap, buf.ctypes.data, buf.size,
                                C.byref(w), C.byref(h), C.byref(c))
            n = w.value * h.value * c.value
            want = ["1", str(w.value), str(h.value), str(c.value), f"{_fnv(buf[:n]):016x}"] \
                if rc == 0 else ["0", "0", "0", "0", f"{0:016x}"]
            assert got[(tag, name)] == want, (tag, name)
            loaded += rc == 0
    # the whole files load (the PFM into the emap only: PerspectiveMap::Load has no PFM branch),
    # the empty file and the cut PNGs / PGM do not
    for name in names:
        whole = "_half" not in name and name != "empty.png"
        assert (got[("E", name)][0] == "1") == whole or name == "rgb_half.jpg", name
    assert loaded >= 13
    assert (out / "gray16.png.8.png").stat().st_size > 0 and (out / "metrics.txt").exists()

    # LoadPfm (Depth.cpp:455-525): flip, then normalise to the file's min..max or cap at 0..10
    mn, mx = pfm.min(), pfm.max()
    for flip in (0, 1):
        v = pfm[::-1] if flip else pfm
        ref = {0: np.minimum(np.maximum(v, 0) / np.float32(10.0), np.float32(10.0)),
               1: (v - mn) / (mx - mn)}
        for norm in (0, 1):
            assert got[(f"F{flip}{norm}", "depth.pfm")] == ["1", "7", "5", "1",
                                                           f"{_fnv(ref[norm]):016x}"], (flip, norm)
    assert got[("F00", "depth_half.pfm")][0] == "0"
