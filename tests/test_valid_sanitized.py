"""The host-only part of the tile-pixel validity rule under AddressSanitizer + UBSan -- CPU only.

csrc/pf_valid.hpp (no HIP include) holds the "LO:HI" parser of PF_TILE_VALID / --tile-valid and the
bookkeeping behind MergeDepthMaps' "[mask]" lines.  tests/cpp/valid_check.cpp (its own main) is
built with -fsanitize=address,undefined -fno-sanitize-recover=all and run as a child process on the
good and the malformed values below, a 1 MB value among them; nothing sanitized is loaded into
Python.  The parsed bounds must be the floats Python parses from the same text, bit for bit, and
panofuse_main must refuse the malformed values before any GPU call."""
import os
import shutil
import struct
import subprocess

import pytest

import panofuse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.dirname(os.path.dirname(panofuse.LIB_PATH))
MAIN = os.path.join(PKG, "bin", "panofuse_main")

GOOD = ["0:inf", "-inf:inf", "0:1", "-INF:+Infinity", "1e-4:0.9999", "-0.5:-0.25", "0x1p-3:1",
        ".5:5.", "-0:1e38", "0:1e39"]  # 1e39 overflows to inf: a bound like any other
BAD = ["", ":", "0", "0:", ":1", "1:0", "0:0", "inf:inf", "nan:1", "0:nan", "0:1:2", "a:b",
       "0:1x", "0 :1", "0: 1", " 0:1", "0:1 ", "0;1", "--:1", "0:inf:", "1" * (1 << 20),
       "0:" + "9" * (1 << 20) + "x", "-inf:-inf"]


def _bits(text):
    return struct.unpack("<I", struct.pack("<f", float.fromhex(text) if "x" in text.lower()
                                           else float(text)))[0]


def _f32(text):
    try:
        return _bits(text)
    except OverflowError:  # struct refuses a double beyond fp32: strtof gives +-inf
        return 0x7F800000 if not text.lstrip().startswith("-") else 0xFF800000


def test_valid_unit_under_asan_ubsan(tmp_path):
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    assert cxx is not None, "no host C++ compiler"
    exe = tmp_path / "valid_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                        os.path.join(PKG, "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "valid_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    cases = tmp_path / "cases.txt"
    cases.write_bytes(("".join(f"ok {t}\n" for t in GOOD) +
                       "".join(f"bad {t}\n" for t in BAD)).encode("latin-1"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1")
    r = subprocess.run([str(exe), str(cases)], capture_output=True, text=True, timeout=300,
                       env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "valid_check ok" in r.stdout and "UNEXPECTED" not in r.stdout
    rows = [ln.split() for ln in r.stdout.splitlines() if ln.split()[:1] in (["ok"], ["bad"])]
    assert len(rows) == len(GOOD) + len(BAD)
    for text, row in zip(GOOD, rows):
        lo, hi = text.split(":")
        assert row == ["ok", "1", f"{_f32(lo):08x}", f"{_f32(hi):08x}"], text
    for row in rows[len(GOOD):]:
        assert row[:2] == ["bad", "0"]
    assert "[mask] tile 1: 96 of 4096 pixels invalid, 40 of 100 samples" in r.stdout


@pytest.mark.parametrize("value", [v for v in BAD if 0 < len(v) < 100])
def test_cli_refuses_a_malformed_range(value, tmp_path):
    env = {k: v for k, v in os.environ.items() if k != "PF_TILE_VALID"}
    r = subprocess.run([MAIN, "0", "a", "b", "c", "d", "--tile-valid", value],
                       capture_output=True, text=True, timeout=30, env=env, cwd=tmp_path)
    assert (r.returncode, r.stdout) == (2, f"bad --tile-valid {value} (want LO:HI, LO < HI)\n")
