"""GPU end-to-end of --layout on the command line: `panofuse_main export --layout midas`,
mode 0 on tiles rendered under the reference's MiDaS table (the documented recipe:
--layout midas --tile-model disparity --tiles output --ext png), the `layout` audit command, and
the refusal of a layout that is neither a name nor a file.  The files follow the pattern of
tests/test_gpu_disp_cli.py; the results are held to the binding, which tests/test_gpu_layouts.py
holds to the oracle."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import panofuse  # noqa: E402
import pf_layouts as PL  # noqa: E402
import pyoracle as O  # noqa: E402
from test_gpu_cli import _png8_write_rgb  # noqa: E402
from test_gpu_disp_cli import _png16_read, _png16_write, _q16, _scene  # noqa: E402
from test_gpu_layouts import _audit_reference  # noqa: E402

PKG = os.path.dirname(os.path.dirname(panofuse.LIB_PATH))
MAIN = os.path.join(PKG, "bin", "panofuse_main")
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "layout_tables.json")))["tables"]
ZR = PL.ZENITH_RANGE
DEV = "cuda:0"


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected on a host without a GPU")


def _jpeg_size(path):
    """(width, height) from the baseline JPEG's SOF0 segment."""
    d = open(path, "rb").read()
    assert d[:2] == b"\xff\xd8"
    pos = 2
    while pos < len(d):
        assert d[pos] == 0xFF
        marker, n = d[pos + 1], struct.unpack(">H", d[pos + 2:pos + 4])[0]
        if marker == 0xC0:
            h, w = struct.unpack(">HH", d[pos + 5:pos + 9])
            return w, h
        pos += 2 + n
    raise AssertionError("no SOF0")


def test_export_midas_tiles(tmp_path):
    _need_gpu()
    (tmp_path / "rgb").mkdir()
    rs = np.random.RandomState(3)
    yy, xx = np.mgrid[0:256, 0:512]
    pano = np.stack([xx * 255 // 511, yy, rs.randint(0, 256, size=(256, 512))], -1).astype(np.uint8)
    _png8_write_rgb(tmp_path / "rgb" / "room7.png", pano)
    # the options in either order, after the two folders
    r = subprocess.run([MAIN, "export", str(tmp_path / "rgb"), str(tmp_path / "tiles"),
                        "--layout", "midas", "--device", "0"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "15 tiles" in r.stdout
    want = {"room7." + "_".join(str(v) for v in f) + ".jpg" for f in GOLDEN["midas"]["fov"]}
    assert set(os.listdir(tmp_path / "tiles")) == want and len(want) == 15
    assert "room7.-2_74_20_78.jpg" in want and "room7.286_362_102_160.jpg" in want
    for name in want:
        assert _jpeg_size(tmp_path / "tiles" / name) == tuple(GOLDEN["midas"]["export_tile"])


def test_mode0_midas_recipe(tmp_path):
    """512 x 256 output, 128 x 64 baseline, 256 x 256 disparity tiles under the midas names in
    output/ as PNG."""
    _need_gpu()
    d = {k: tmp_path / k for k in ("rgb", "gt", "base", "result_hohonet", "output")}
    for p in d.values():
        p.mkdir()
    tw = th = 256
    lay = PL.midas_layout(tw, th)
    tiles, gt, base, disp = _scene(lay, 20261015 + 99, 512, 128)
    raw = "scene01_rgb"
    (d["rgb"] / (raw + ".jpg")).write_bytes(b"\xff\xd8")  # only the name is used
    gq, bq, tq = _q16(gt), _q16(base), _q16(disp)
    _png16_write(d["gt"] / (raw.replace("_rgb", "_depth") + ".png"), gq)
    _png16_write(d["base"] / (raw + ".depth.png"), bq)  # hohonet naming (Main.cpp:512-516)
    names = PL.tile_names(lay)
    assert names[0] == "-2_74_20_78"
    for t in range(lay.ntiles):
        _png16_write(d["output"] / f"{raw}.{names[t]}.png",
                     tq[t * tw * th:(t + 1) * tw * th].reshape(th, tw))
    cmd = [MAIN, "0", str(d["rgb"]), str(d["gt"]), str(d["base"]), str(d["result_hohonet"]),
           "--tile-model", "disparity", "--tiles", str(d["output"]), "--ext", "png",
           "--width", "512", "--layout", "midas"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    want_audit = _audit_reference(lay, 512)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("[layout]")]
    assert lines == [f"[layout] level {lv} ({a['w']}x{a['h']}): {a['taps_outside']} taps outside "
                     "their tile (clamped)" for lv, a in enumerate(want_audit)
                     if a["taps_outside"] > 0]
    assert lines[0] == "[layout] level 0 (128x64): 217 taps outside their tile (clamped)"
    got = _png16_read(d["result_hohonet"] / (raw + ".png"))
    assert got.shape == (256, 512)

    # the facade call (the binding) on the pixels the files decode to
    fz = panofuse.Fuser(0)
    fz.set_tiles(lay)
    t_emap = torch.from_numpy(bq.astype(np.float32) / np.float32(65535.0))[None].to(DEV)
    t_tiles = torch.from_numpy(tq.astype(np.float32) / np.float32(65535.0))[None].to(DEV)
    out = torch.zeros((1, 256, 512), dtype=torch.int16, device=DEV)
    fz.merge_disparity(t_emap.contiguous(), t_tiles.contiguous(), out, ZR)
    fz.synchronize()
    assert np.array_equal(got, out.cpu().numpy().view(np.uint16)[0])

    # the same files through a layout file with midas' degrees: the same tile names
    (d["result_hohonet"] / (raw + ".png")).unlink()
    g = GOLDEN["midas"]
    lf = tmp_path / "midas_degrees.txt"
    lf.write_text("# midas, from its integer degrees\n" +
                  "".join("%d %d %d %d %d %d %d %d\n" % (*f, *rg)
                          for f, rg in zip(g["fov"], g["range"])))
    r = subprocess.run(cmd[:-1] + [str(lf)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert _png16_read(d["result_hohonet"] / (raw + ".png")).shape == (256, 512)

    # without --layout the command looks for the leres names and finds no tiles
    (d["result_hohonet"] / (raw + ".png")).unlink()
    r = subprocess.run(cmd[:-2], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0, r.stdout + r.stderr
    assert not (d["result_hohonet"] / (raw + ".png")).exists()
    assert "[layout]" not in r.stdout


def test_layout_command(tmp_path):
    _need_gpu()
    r = subprocess.run([MAIN, "layout", "fold3", "--width", "512", "--tile-size", "256x192"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    want = [f"LEVEL {lv} {a['w']} {a['h']} {a['h0']} {a['h1']} {a['taps_outside']} "
            f"{a['taps_clamped']} {a['covered']} {a['uncovered_interior']} {a['max_cover']} "
            f"{a['seam']}" for lv, a in enumerate(_audit_reference(PL.fold3_layout(256, 192), 512))]
    assert [ln for ln in r.stdout.splitlines() if ln.startswith("LEVEL")] == want
    assert want[0].split()[6] == "46" and want[2].split()[9] == "511"
    # a layout pf_set_tiles rejects: a window with no width
    bad = tmp_path / "flat.txt"
    bad.write_text("10 10 40 120 80 0 60 120\n")
    r = subprocess.run([MAIN, "layout", str(bad)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "degenerate window" in r.stdout, r.stdout + r.stderr


def test_bad_layout_exits_2(tmp_path):
    _need_gpu()
    for cmd in ([MAIN, "0", "a", "b", "c", "d", "--layout", "nosuch"],
                [MAIN, "export", "a", "b", "--layout", "nosuch"],
                [MAIN, "layout", "nosuch"]):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (cmd, r.stdout + r.stderr)
        assert "neither a known name" in r.stdout
    seven = tmp_path / "seven.txt"
    seven.write_text("0 90 45 135 90 0 60\n")
    r = subprocess.run([MAIN, "export", "a", "b", "--layout", str(seven)], capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 2 and "want eight numbers" in r.stdout
