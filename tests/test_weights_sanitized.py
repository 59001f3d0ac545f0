"""The host-only part of the per-pixel tile weights under AddressSanitizer + UBSan -- CPU only.

csrc/pf_weights.hpp (no HIP include) holds the "tent" / "files:SUFFIX" parser of PF_TILE_WEIGHTS /
--tile-weights, the weight-file name, the size check's message and MergeDepthMaps' "[weights]"
lines.  tests/cpp/weights_check.cpp (its own main) is built with -fsanitize=address,undefined
-fno-sanitize-recover=all and run as a child process on the good and the malformed values below, a
1 MB value among them; nothing sanitized is loaded into Python.  panofuse_main must refuse the
malformed values, and the flag next to an option it cannot go with, before any GPU call."""
import os
import shutil
import subprocess

import pytest

import panofuse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.dirname(os.path.dirname(panofuse.LIB_PATH))
MAIN = os.path.join(PKG, "bin", "panofuse_main")

GOOD = {"tent": (1, ""), "off": (0, ""), "files:.w.pfm": (2, ".w.pfm"), "files:_conf.png": (2, "_conf.png"),
        "files:files:": (2, "files:"), "files:" + "w" * (1 << 20): (2, "w" * (1 << 20)),
        "files: .pfm": (2, " .pfm")}
BAD = ["", "Tent", "tent ", " tent", "tents", "files", "files:", "file:.pfm", "files:/etc/passwd",
       "files:../x.pfm", "files:a\\b", "1", "files;.pfm", "t" * (1 << 20), "tent:files:.pfm"]
# what --tile-weights cannot go with: (options, the name in the message)
CLASHES = [(["--tile-valid", "0:inf"], "--tile-valid"),
           (["--reg-loss", "huber:0.1"], "--reg-loss"),
           (["--tile-depth", "planar"], "--tile-depth planar"),
           (["--reg-consistent", "1"], "--reg-consistent"),
           (["--tile-model", "disparity"], "--tile-model disparity"),
           (["--global-align"], "--global-align"),
           (["--fusion", "smoothing"], "--fusion smoothing"),
           (["--fusion", "stitch"], "--fusion stitch"),
           (["--check-laplacian"], "--check-laplacian")]
ENV_DROP = ("PF_TILE_WEIGHTS", "PF_TILE_VALID", "PF_REG_LOSS", "PF_TILE_DEPTH", "PF_TILE_MODEL",
            "PF_FUSION", "PF_REG_CONSISTENT", "PF_GLOBAL_ALIGN", "PF_CHECK_LAPLACIAN")


def test_weights_unit_under_asan_ubsan(tmp_path):
    cxx = next((c for c in ("g++", "c++", "clang++") if shutil.which(c)), None)
    assert cxx is not None, "no host C++ compiler"
    exe = tmp_path / "weights_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", os.path.join(PKG, "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "weights_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    cases = tmp_path / "cases.txt"
    cases.write_bytes(("".join(f"ok {t}\n" for t in GOOD) +
                       "".join(f"bad {t}\n" for t in BAD)).encode("latin-1"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1")
    r = subprocess.run([str(exe), str(cases)], capture_output=True, text=True, timeout=300,
                       env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "weights_check ok" in r.stdout and "UNEXPECTED" not in r.stdout
    rows = [ln for ln in r.stdout.splitlines() if ln.split(" ")[0] in ("ok", "bad")]
    assert len(rows) == len(GOOD) + len(BAD)
    for (text, (mode, suffix)), row in zip(GOOD.items(), rows):
        assert row == f"ok 1 {mode} {suffix}", text[:40]
    for row in rows[len(GOOD):]:
        assert row == "bad 0 9 kept"
    assert "[weights] tile 3: 1234 of 4096 samples used, sum w 617.25" in r.stdout
    assert "[weights] tile 0: 0 of 0 samples used, sum w 0" in r.stdout


def _main(tmp_path, *opts):
    env = {k: v for k, v in os.environ.items() if k not in ENV_DROP}
    return subprocess.run([MAIN, "0", "a", "b", "c", "d", *opts], capture_output=True, text=True,
                          timeout=30, env=env, cwd=tmp_path)


@pytest.mark.parametrize("value", [v for v in BAD if 0 < len(v) < 100] + ["off"])
def test_cli_refuses_a_malformed_value(value, tmp_path):
    r = _main(tmp_path, "--tile-weights", value)
    assert (r.returncode, r.stdout) == (2, f"bad --tile-weights {value} (want tent or "
                                           f"files:SUFFIX)\n")


@pytest.mark.parametrize("opts,name", CLASHES, ids=[c[1].replace(" ", "_") for c in CLASHES])
@pytest.mark.parametrize("first", [True, False], ids=["before", "after"])
def test_cli_refuses_the_flag_next_to_what_it_cannot_go_with(opts, name, first, tmp_path):
    mine = ["--tile-weights", "tent"]
    r = _main(tmp_path, *(mine + opts if first else opts + mine))
    assert (r.returncode, r.stdout) == (
        2, f"--tile-weights registers and fuses with per-pixel weights: not with {name}\n")
