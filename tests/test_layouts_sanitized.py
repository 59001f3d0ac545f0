"""The layout tables and the layout-file parser under AddressSanitizer + UBSan -- CPU only.

csrc/pf_layouts.cpp is a host-only unit (no HIP include), so the host compiler builds it alone.
tests/cpp/layouts_check.cpp (its own main) links it with
-fsanitize=address,undefined -fno-sanitize-recover=all and parses the good and the malformed
files of tests/test_layouts.py plus a 1 MB line (as a comment, as one token, as a million numbers)
and a file of 5000 tiles.  It runs as a child process; nothing sanitized is loaded into Python.
Every result must equal the unsanitized library's (pfd_layout), by tile count and by a hash of
the tiles' bits, so the sanitized run took the same paths."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import panofuse
import pf_layouts as PL
from test_layouts import GOOD, MALFORMED, _file_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.dirname(os.path.dirname(panofuse.LIB_PATH))


def _fnv(fovs, ranges):
    h = 1469598103934665603
    for b in np.concatenate([fovs, ranges], axis=1).astype(np.float32).tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_layouts_unit_under_asan_ubsan(tmp_path):
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    assert cxx is not None, "no host C++ compiler"
    exe = tmp_path / "layouts_check"
    csrc = os.path.join(PKG, "csrc")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc,
                        os.path.join(ROOT, "tests", "cpp", "layouts_check.cpp"),
                        os.path.join(csrc, "pf_layouts.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]

    d = tmp_path / "files"
    d.mkdir()
    files = {"good_fold4.txt": _file_text("fold4"), "good_leres.txt": _file_text("leres"),
             "good_max.txt": GOOD * PL.MAX_TILES,
             "good_noeol.txt": "  +0. 9e1 .45e2 135.0 90 -0 60 120 # no newline at the end",
             "good_long_comment.txt": GOOD + "#" + "x" * (1 << 20) + "\n" + GOOD,
             "bad_long_token.txt": "0 90 45 135 90 0 60 " + "1" * (1 << 20) + "\n",
             "bad_long_line.txt": "7 " * (1 << 19) + "\n",
             "bad_5000_tiles.txt": GOOD * 5000,
             "bad_binary.txt": "0 90 45 135 90 0 60 12\x000\n"}
    files.update({f"bad_{k}.txt": v for k, v in MALFORMED.items()})
    for name, text in files.items():
        (d / name).write_bytes(text.encode("latin-1"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1")
    r = subprocess.run([str(exe), str(d)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "layouts_check ok" in r.stdout
    got = {ln.split()[0]: (int(ln.split()[1]), int(ln.split()[2], 16))
           for ln in r.stdout.splitlines() if len(ln.split()) == 3}

    L = C.CDLL(os.path.join(PKG, "lib", "libpanofuse_depth.so"))
    L.pfd_layout.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_int]
    for name in ["leres", "midas", "fold4", "fold3"] + sorted(files):
        f = np.zeros((PL.MAX_TILES, 4), np.float32)
        rg = np.zeros((PL.MAX_TILES, 4), np.float32)
        spec = name if name not in files else str(d / name)
        n = L.pfd_layout(os.fsencode(spec), f.ctypes.data, rg.ctypes.data, PL.MAX_TILES)
        assert n == got[name][0], name
        assert (n > 0) == (name not in files or name.startswith("good_")), name
        assert _fnv(f[:max(n, 0)], rg[:max(n, 0)]) == got[name][1], name
