"""The host-only part of the planar-depth tiles under AddressSanitizer + UBSan -- CPU only.

csrc/pf_ray.hpp (no HIP include) holds the ray-factor table builder that pf_set_tiles runs and the
parser of PF_TILE_DEPTH / --tile-depth.  tests/cpp/ray_check.cpp (its own main) is built with
-fsanitize=address,undefined -fno-sanitize-recover=all and run as a child process; nothing
sanitized is loaded into Python.  The cases: a tile one pixel wide, one a pixel high, a window given
right-to-left, and 32 tiles of mixed sizes packed into one exactly sized buffer, as pf_set_tiles
packs them.  The tables must be tests/planar_ref.py's (within the 4 ulp the two tan calls may
differ by), the factor of the first pixel its float32 value bit for bit."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import panofuse
import planar_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.dirname(os.path.dirname(panofuse.LIB_PATH))

PARSE = [("ray", 0), ("planar", 1), ("", -1), ("Planar", -1), ("planar ", -1), (" ray", -1),
         ("rays", -1), ("ra", -1), ("1", -1), ("p" * (1 << 20), -1)]


def _tiles():
    rng = np.random.default_rng(20261020)
    t = [((0.3, 1.5, 0.4, 1.2), 1, 7), ((0.3, 1.5, 0.4, 1.2), 9, 1),
         ((1.5, 0.3, 1.2, 0.4), 9, 7), ((0.0, 0.0, 1.0, 1.0), 4, 4)]
    for _ in range(32):
        a0, z0 = rng.uniform(0, 5), rng.uniform(0.3, 1.5)
        t.append(((a0, a0 + rng.uniform(0.2, 2.4), z0, z0 + rng.uniform(0.2, 1.4)),
                  int(rng.integers(1, 300)), int(rng.integers(1, 300))))
    return [(tuple(float(np.float32(v)) for v in win), w, h) for win, w, h in t]


def test_ray_tables_under_asan_ubsan(tmp_path):
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    assert cxx is not None, "no host C++ compiler"
    exe = tmp_path / "ray_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                        os.path.join(PKG, "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "ray_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    tiles = _tiles()
    cases = tmp_path / "cases.txt"
    cases.write_text("".join("tile " + " ".join(float(v).hex() for v in win) + f" {w} {h}\n"
                             for win, w, h in tiles)
                     + "".join(f"parse {text}\n" for text, _ in PARSE))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1")
    r = subprocess.run([str(exe), str(cases)], capture_output=True, text=True, timeout=300,
                       env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "ray_check ok" in r.stdout and "UNEXPECTED" not in r.stdout
    lines = r.stdout.splitlines()
    parsed = [int(ln.split()[1]) for ln in lines if ln.startswith("parse ")]
    assert parsed == [want for _, want in PARSE]
    heads = [i for i, ln in enumerate(lines) if ln.startswith("tile ")]
    assert len(heads) == len(tiles)
    for (win, w, h), i in zip(tiles, heads):
        tag, gw, gh, k00 = lines[i].split()
        assert (int(gw), int(gh)) == (w, h)
        tab = np.array([int(x, 16) for x in lines[i + 1].split()], np.uint64).view(np.float64)
        assert tab.size == w + h
        cu, rv = P.tables(win, w, h)
        want = np.concatenate([cu, rv])
        ulp = np.abs(tab.view(np.int64) - want.view(np.int64)).max()
        assert ulp <= 4, (win, w, h, int(ulp))
        k = P.kf(tab[:w], tab[w:])[0, 0]
        assert int(k00, 16) == int(k.view(np.uint32))
        if w == 1:
            assert tab[0] == 0.0
        if h == 1:
            assert tab[w] == 0.0
    # the window given right-to-left has the tables of the same window left-to-right
    a, b = heads[2], heads[1]
    assert lines[a + 1].split()[:9] == lines[b + 1].split()[:9]


@pytest.mark.parametrize("value", ["", "Planar", "plane", "ray ", "1", "planar:1"])
def test_cli_refuses_a_bad_tile_depth(value, tmp_path):
    env = {k: v for k, v in os.environ.items() if k != "PF_TILE_DEPTH"}
    r = subprocess.run([os.path.join(PKG, "bin", "panofuse_main"), "0", "a", "b", "c", "d",
                        "--tile-depth", value],
                       capture_output=True, text=True, timeout=30, env=env, cwd=tmp_path)
    assert (r.returncode, r.stdout) == (2, f"bad --tile-depth {value} (want planar or ray)\n")
