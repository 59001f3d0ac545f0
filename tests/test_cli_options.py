"""panofuse_main's option handling, pinned literally -- CPU only.

Every argument list here ends before the first HIP call (a usage line, a rejected option, a file
that does not load), so the cases run in milliseconds on any host.  Exit status and stdout are
compared as they are: the wording, the status (1 for a usage or load error, 2 for a rejected
option) and the CLI's quirks -- an unknown first word exits 0 silently, mode 0 ignores a trailing
option that lacks its value while export / layout / cmp answer `option ... needs a value`, cmp
loads its files before it selects the device."""
import os
import struct
import subprocess
import zlib

import pytest

import panofuse

PKG = os.path.dirname(os.path.dirname(panofuse.LIB_PATH))
MAIN = os.path.join(PKG, "bin", "panofuse_main")
SWITCHES = ("PF_FUSION", "PF_SAVE_STITCH", "PF_CHECK_LAPLACIAN", "PF_GLOBAL_ALIGN", "PF_LAYOUT",
            "PF_EDGE_METRICS", "PF_TILE_MODEL", "PF_METRICS_ORDER")

U_EXPORT = "export <rgb_dir> <tile_dir> [--device D] [--layout NAME|FILE]"
U_LAYOUT = "layout NAME|FILE [--width W] [--tile-size WxH] [--device D]"
U_LAP = "lap <gt_file> <given_file> [--device D]"
U_CMP = ("cmp <gt_file> <given_file> [--disp] [--align 0|1|2] [--no-cap] [--save FILE]"
         " [--device D] [--metrics-order tree|sequential]")
USAGE = (
    "usage: {m} 0 <rgb_dir> <gt_dir> <baseline_dir> <result_dir> [--tiles DIR]"
    " [--ext auto|jpg|png] [--width W] [--device D] [--shard R/N]"
    " [--metrics-order tree|sequential] [--edge-metrics] [--tile-model depth|disparity]"
    " [--global-align] [--layout NAME|FILE] [--fusion laplacian|smoothing|stitch] [--save-stitch]"
    " [--check-laplacian]\n"
    "         (MiDaS disparity tiles, the reference's folder convention: --layout midas"
    " --tile-model disparity --tiles output --ext png)\n"
    "         (--layout: leres (default), midas, fold4, fold3, or a file of lines"
    " `faz0 faz1 fzen0 fzen1 raz0 raz1 rzen0 rzen1` in degrees)\n"
    "       {m} " + U_EXPORT + "\n"
    "       {m} " + U_LAYOUT + "\n"
    "       {m} " + U_LAP + "\n"
    "       {m} " + U_CMP + "\n")
NOSUCH = ("layout 'nosuch' is neither a known name (leres, midas, fold4, fold3) nor a usable "
          "layout file: cannot open layout file nosuch\n")
NEEDS = "--check-laplacian needs --fusion laplacian (got stitch)\n"
M0 = ["0", "a", "b", "c", "d"]

CASES = [
    ([], 0, USAGE),
    (["frobnicate"], 0, ""),
    (["frobnicate", "--fusion", "median"], 0, ""),
    # too few arguments
    (["export"], 1, "usage: {m} " + U_EXPORT + "\n"),
    (["export", "a"], 1, "usage: {m} " + U_EXPORT + "\n"),
    (["layout"], 1, "usage: {m} " + U_LAYOUT + "\n"),
    (["lap", "a"], 1, "usage: {m} " + U_LAP + "\n"),
    (["cmp", "a"], 1, "usage: {m} " + U_CMP + "\n"),
    (["0", "a", "b", "c"], 1, "[CreateDepthPanormas] error: need argc>=6\n"),
    # an unknown option
    (["export", "a", "b", "--bogus", "1"], 2, "unknown option --bogus\n"),
    (["layout", "leres", "--bogus", "1"], 2, "unknown option --bogus\n"),
    (["cmp", "a", "b", "--bogus", "1"], 2, "unknown option --bogus\n"),
    (M0 + ["--bogus", "1"], 2, "unknown option --bogus\n"),
    # an option without its value: export, layout and cmp refuse it ...
    (["export", "a", "b", "--device"], 2, "option --device needs a value\n"),
    (["export", "a", "b", "--layout"], 2, "option --layout needs a value\n"),
    (["layout", "leres", "--width"], 2, "option --width needs a value\n"),
    (["cmp", "a", "b", "--align"], 2, "option --align needs a value\n"),
    (["cmp", "a", "b", "--bogus"], 2, "option --bogus needs a value\n"),
    # ... mode 0 drops it silently (the status and the line are the consistency rule's)
    (M0 + ["--check-laplacian", "--fusion", "stitch", "--tiles"], 2, NEEDS),
    # rejected values
    (["layout", "leres", "--tile-size", "1x"], 2, "bad --tile-size 1x (want WxH)\n"),
    (["cmp", "a", "b", "--align", "3"], 2, "bad --align 3 (want 0, 1 or 2)\n"),
    (["cmp", "a", "b", "--disp", "--no-cap", "--align", "-1"], 2,
     "bad --align -1 (want 0, 1 or 2)\n"),
    (["cmp", "a", "b", "--metrics-order", "x"], 2,
     "bad --metrics-order x (want tree or sequential)\n"),
    (M0 + ["--metrics-order", "x"], 2, "bad --metrics-order x (want tree or sequential)\n"),
    (M0 + ["--tile-model", "x"], 2, "bad --tile-model x (want depth or disparity)\n"),
    (M0 + ["--fusion", "median"], 2, "bad --fusion median (want laplacian, smoothing or stitch)\n"),
    (M0 + ["--shard", "3/2"], 2, "bad --shard 3/2 (want R/N, 0 <= R < N)\n"),
    (M0 + ["--layout", "nosuch"], 2, "bad --layout: " + NOSUCH),
    (["export", "a", "b", "--layout", "nosuch"], 2, "bad --layout: " + NOSUCH),
    (["layout", "nosuch"], 2, "bad layout: " + NOSUCH),
    # the consistency rule, in both orders
    (M0 + ["--check-laplacian", "--fusion", "stitch"], 2, NEEDS),
    (M0 + ["--fusion", "stitch", "--check-laplacian"], 2, NEEDS),
    (M0 + ["--fusion", "smoothing", "--check-laplacian"], 2,
     "--check-laplacian needs --fusion laplacian (got smoothing)\n"),
]


def _run(args, cwd):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    return subprocess.run([MAIN] + args, capture_output=True, text=True, timeout=30, env=env,
                          cwd=cwd)


@pytest.mark.parametrize("args,status,out", CASES, ids=[" ".join(c[0]) or "none" for c in CASES])
def test_early_exits(args, status, out, tmp_path):
    r = _run(args, tmp_path)
    assert (r.returncode, r.stdout) == (status, out.replace("{m}", MAIN)), r.stderr


def _png8(path, w, h):
    def chunk(t, d):
        return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d))
    raw = b"".join(b"\0" + bytes(range(y * w, y * w + w)) for y in range(h))
    path.write_bytes(b"\x89PNG\r\n\x1a\n" +
                     chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0)) +
                     chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b""))


def test_cmp_loads_before_it_selects_the_device(tmp_path):
    """A file that does not load ends cmp with status 1 and the reference's two lines, on a host
    with or without a GPU: the loads come before hipSetDevice."""
    ok, missing = tmp_path / "ok.png", tmp_path / "missing.png"
    _png8(ok, 4, 2)
    r = _run(["cmp", str(missing), str(ok)], tmp_path)
    assert (r.returncode, r.stdout) == (
        1, f"[EquirectangularMap::Load] failed: cannot open {missing}\n"
           f"cannot load emap_gt? {missing}\n"), r.stderr
    r = _run(["cmp", str(ok), str(missing), "--device", "99"], tmp_path)
    assert (r.returncode, r.stdout) == (
        1, f"[EquirectangularMap::Load] failed: cannot open {missing}\n"
           f"cannot load emap_baseline? {missing}\n"), r.stderr
