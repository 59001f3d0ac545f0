"""The host-only part of the disparity tiles' weights under AddressSanitizer + UBSan -- CPU only.

csrc/pf_disp_weights.hpp (no HIP include) holds the "tent" / "files:SUFFIX" / "range:LO:HI" parser
of PF_DISPARITY_WEIGHTS / --disparity-weights and the names of what the switch cannot go with.
tests/cpp/disp_weights_check.cpp (its own main) is built with -fsanitize=address,undefined
-fno-sanitize-recover=all and run as a child process on the good and the malformed values below, a
1 MB value among them; nothing sanitized is loaded into Python.  panofuse_main must refuse the
malformed values, the flag without --tile-model disparity, and the flag next to an option it
cannot go with, before any GPU call."""
import os
import shutil
import subprocess

import pytest

import panofuse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.dirname(os.path.dirname(panofuse.LIB_PATH))
MAIN = os.path.join(PKG, "bin", "panofuse_main")

# text -> (mode, lo, hi, suffix) as the check program prints them
GOOD = {"tent": (1, "0", "0", ""), "off": (0, "0", "0", ""),
        "files:.w.pfm": (2, "0", "0", ".w.pfm"),
        "files:" + "w" * (1 << 20): (2, "0", "0", "w" * (1 << 20)),
        "range:0:inf": (3, "0", "inf", ""), "range:-inf:inf": (3, "-inf", "inf", ""),
        "range:0.25:0.75": (3, "0.25", "0.75", ""), "range:1e-4:1": (3, "0.0001", "1", "")}
BAD = ["", "Tent", "tent ", " tent", "files", "files:", "files:/etc/passwd", "files:a\\b",
       "range", "range:", "range:0", "range:0:", "range::1", "range:1:0", "range:0:0",
       "range:nan:1", "range:0:1:2", "range:a:b", "range: 0:1", "range:0:1 ", "Range:0:1",
       "range;0:1", "1", "t" * (1 << 20), "range:" + "9" * (1 << 20), "tent:range:0:1"]
# what --disparity-weights cannot go with: (options, the name in the message)
CLASHES = [(["--tile-valid", "0:inf"], "--tile-valid"),
           (["--reg-loss", "huber:0.1"], "--reg-loss"),
           (["--reg-consistent", "1"], "--reg-consistent"),
           (["--global-align"], "--global-align"),
           (["--fusion", "smoothing"], "--fusion smoothing"),
           (["--fusion", "stitch"], "--fusion stitch"),
           (["--check-laplacian"], "--check-laplacian"),
           (["--tile-weights", "tent"], "--tile-weights")]
ENV_DROP = ("PF_DISPARITY_WEIGHTS", "PF_TILE_WEIGHTS", "PF_TILE_VALID", "PF_REG_LOSS",
            "PF_TILE_DEPTH", "PF_TILE_MODEL", "PF_FUSION", "PF_REG_CONSISTENT", "PF_GLOBAL_ALIGN",
            "PF_CHECK_LAPLACIAN")
MESSAGE = "--disparity-weights fits and fuses disparity tiles with per-pixel weights: not with "


def test_parser_under_asan_ubsan(tmp_path):
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    assert cxx is not None, "no host C++ compiler"
    exe = tmp_path / "disp_weights_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", os.path.join(PKG, "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "disp_weights_check.cpp"), "-o",
                        str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    cases = tmp_path / "cases.txt"
    cases.write_bytes(("".join(f"ok {t}\n" for t in GOOD) +
                       "".join(f"bad {t}\n" for t in BAD)).encode("latin-1"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1")
    r = subprocess.run([str(exe), str(cases)], capture_output=True, text=True, timeout=300,
                       env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "disp_weights_check ok" in r.stdout and "UNEXPECTED" not in r.stdout
    rows = [ln for ln in r.stdout.splitlines() if ln.split(" ")[0] in ("ok", "bad")]
    assert len(rows) == len(GOOD) + len(BAD)
    for (text, (mode, lo, hi, suffix)), row in zip(GOOD.items(), rows):
        assert row == f"ok 1 {mode} {lo} {hi} {suffix}", text[:40]
    for row in rows[len(GOOD):]:
        assert row == "bad 0 9 -5 5 kept"
    for _, name in CLASHES:
        assert MESSAGE + name + " | " in r.stdout, name


def _main(tmp_path, *opts):
    env = {k: v for k, v in os.environ.items() if k not in ENV_DROP}
    return subprocess.run([MAIN, "0", "a", "b", "c", "d", *opts], capture_output=True, text=True,
                          timeout=30, env=env, cwd=tmp_path)


@pytest.mark.parametrize("value", [v for v in BAD if 0 < len(v) < 100] + ["off"])
def test_cli_refuses_a_malformed_value(value, tmp_path):
    r = _main(tmp_path, "--tile-model", "disparity", "--disparity-weights", value)
    assert (r.returncode, r.stdout) == (2, f"bad --disparity-weights {value} (want tent, "
                                           f"files:SUFFIX or range:LO:HI)\n")


@pytest.mark.parametrize("spec", ["tent", "range:0:inf"])
def test_cli_refuses_the_flag_without_disparity_tiles(spec, tmp_path):
    for opts in (["--disparity-weights", spec],
                 ["--disparity-weights", spec, "--tile-model", "depth"],
                 ["--tile-model", "depth", "--disparity-weights", spec]):
        r = _main(tmp_path, *opts)
        assert (r.returncode, r.stdout) == (2, MESSAGE + "--tile-model depth\n"), opts


@pytest.mark.parametrize("opts,name", CLASHES, ids=[c[1].replace(" ", "_") for c in CLASHES])
@pytest.mark.parametrize("first", [True, False], ids=["before", "after"])
def test_cli_refuses_the_flag_next_to_what_it_cannot_go_with(opts, name, first, tmp_path):
    mine = ["--tile-model", "disparity", "--disparity-weights", "range:0:inf"]
    r = _main(tmp_path, *(mine + opts if first else opts + mine))
    assert (r.returncode, r.stdout) == (2, MESSAGE + name + "\n")
