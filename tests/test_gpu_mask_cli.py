"""GPU end-to-end of the tile-pixel validity rule on the command line and through the facade.

Mode 0 on a C1-sized folder (512x256 output, 128x64 baseline, the default table's 15 tiles at
256x247 as 16-bit PNGs, the pattern of tests/test_gpu_disp_cli.py) whose tile files have a black
region: with --tile-valid 0:inf the result PNG equals the binding's output byte for byte and the
"[mask]" lines are printed; without the flag no "[mask]" line is printed.  The flag is refused
with --tile-model disparity and --fusion smoothing.  tests/cpp/valid_link.cpp calls
SetTileValidity from compiled C++ against the binding on the same hand-filled maps."""
import os
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import panofuse  # noqa: E402
import pf_layouts as PL  # noqa: E402
import pf_synth  # noqa: E402
import pyoracle as O  # noqa: E402
from test_gpu_disp_cli import _png16_read, _png16_write, _q16  # noqa: E402

PKG = os.path.dirname(os.path.dirname(panofuse.LIB_PATH))
MAIN = os.path.join(PKG, "bin", "panofuse_main")
LINK = os.path.join(PKG, "bin", "pf_valid_link")
ZR = PL.ZENITH_RANGE
DEV = "cuda:0"
RAW = "scene01_rgb"
TW, TH = 256, 247
# black regions: a bar across tile 2, a block of tile 9, all of tile 12
BLACK = {2: (slice(0, 60), slice(0, TW)), 9: (slice(80, 200), slice(40, 160)),
         12: (slice(0, TH), slice(0, TW))}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected on a host without a GPU")


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    _need_gpu()
    root = tmp_path_factory.mktemp("mask_cli")
    d = {k: root / k for k in ("rgb", "gt", "base", "tiles")}
    for p in d.values():
        p.mkdir()
    lay = PL.leres_layout(TW, TH)
    tiles, total = O.make_tiles(lay)
    seeds = pf_synth.seeds_for(1, 20261015 + 55)
    gt = pf_synth.scene_depth(seeds, 512, 256)[0].numpy()
    base = pf_synth.baseline_emap(seeds, 128, 64)[0].numpy()
    depth = O.warp_depth(gt, tiles, total, O.responses(pf_synth.responses(seeds, lay.ntiles)))
    (d["rgb"] / (RAW + ".jpg")).write_bytes(b"\xff\xd8")  # only the name is used
    tq = _q16(depth).reshape(lay.ntiles, TH, TW).copy()
    assert (tq > 0).all()
    for t, (ys, xs) in BLACK.items():
        tq[t, ys, xs] = 0
    bq = _q16(base)
    _png16_write(d["gt"] / (RAW.replace("_rgb", "_depth") + ".png"), _q16(gt))
    _png16_write(d["base"] / (RAW + ".depth.png"), bq)
    names = PL.tile_names(lay)
    for t in range(lay.ntiles):
        _png16_write(d["tiles"] / f"{RAW}.{names[t]}.png", tq[t])

    def run(tag, *opts):
        res = root / tag / "result_hohonet"
        res.mkdir(parents=True)
        cmd = [MAIN, "0", str(d["rgb"]), str(d["gt"]), str(d["base"]), str(res), "--tiles",
               str(d["tiles"]), "--ext", "png", "--width", "512"] + list(opts)
        env = {k: v for k, v in os.environ.items() if k != "PF_TILE_VALID"}
        return subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=env), res

    t_emap = torch.from_numpy(bq.astype(np.float32) / np.float32(65535.0))[None].to(DEV)
    t_tiles = torch.from_numpy((tq.astype(np.float32) / np.float32(65535.0)).reshape(1, -1)).to(DEV)
    return run, lay, t_emap.contiguous(), t_tiles.contiguous(), tq


def test_tile_valid_flag(folder):
    run, lay, t_emap, t_tiles, tq = folder
    r, res = run("masked", "--tile-valid", "0:inf")
    assert r.returncode == 0, r.stdout + r.stderr
    got = _png16_read(res / (RAW + ".png"))

    fz = panofuse.Fuser(0)
    fz.set_tiles(lay)
    fz.set_tile_validity(lo=0.0)
    out = torch.zeros((1, 256, 512), dtype=torch.int16, device=DEV)
    fz.merge(t_emap, t_tiles, out, ZR)
    counts = fz.tile_valid_counts(t_emap, t_tiles, ZR)
    fz.set_tile_validity(None, None)
    totals = fz.tile_valid_counts(t_emap, t_tiles, ZR)
    fz.synchronize()
    want = out.cpu().numpy().view(np.uint16)[0]
    assert np.array_equal(got, want)
    lv = O.level_dims(512, 256, ZR, 2)
    assert (want[lv.h0:lv.h1 + 1] == 0).mean() < 0.01, "the masked panorama must fill its band"
    # the binding's file is the command's file, byte for byte
    ref_png = res.parent / "binding.png"
    _png16_write(ref_png, want)
    assert _png16_read(ref_png).tobytes() == got.tobytes()

    cn, tt = counts.cpu().numpy()[0], totals.cpu().numpy()[0]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("[mask]")]
    want_lines = [f"[mask] tile {t}: {tt[t, 1] - cn[t, 1]} of {tt[t, 1]} pixels invalid, "
                  f"{tt[t, 0] - cn[t, 0]} of {tt[t, 0]} samples" for t in sorted(BLACK)]
    assert lines == want_lines, r.stdout
    for t in sorted(BLACK):
        assert tt[t, 1] == TW * TH and tt[t, 1] - cn[t, 1] == int((tq[t] == 0).sum())
    assert cn[12, 0] == 0 and cn[12, 1] == 0
    fz.close()


def test_without_the_flag_nothing_changes(folder):
    run, lay, t_emap, t_tiles, _ = folder
    r, res = run("plain")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "[mask]" not in r.stdout
    fz = panofuse.Fuser(0)
    fz.set_tiles(lay)
    out = torch.zeros((1, 256, 512), dtype=torch.int16, device=DEV)
    fz.merge(t_emap, t_tiles, out, ZR)
    fz.synchronize()
    assert np.array_equal(_png16_read(res / (RAW + ".png")), out.cpu().numpy().view(np.uint16)[0])
    fz.close()


@pytest.mark.parametrize("opts,entry", [(("--tile-model", "disparity"), "pf_register_disparity"),
                                        (("--fusion", "smoothing"), "pf_solve_smoothing")])
def test_flag_is_refused_where_it_cannot_hold(folder, opts, entry):
    run = folder[0]
    r, res = run("refused_" + opts[1], "--tile-valid", "-inf:inf", *opts)
    assert "pf_set_tile_validity" in r.stdout and entry in r.stdout, r.stdout + r.stderr
    assert not (res / (RAW + ".png")).exists()


def test_stitch_fusion_under_the_flag(folder):
    run, lay, t_emap, t_tiles, _ = folder
    r, res = run("stitch", "--tile-valid", "0:inf", "--fusion", "stitch")
    assert r.returncode == 0, r.stdout + r.stderr
    fz = panofuse.Fuser(0)
    fz.set_tiles(lay)
    fz.set_tile_validity(lo=0.0)
    cf = torch.zeros((1, lay.ntiles, 4), dtype=torch.float32, device=DEV)
    fz.register(t_emap, t_tiles, ZR, degree=3, apply=False, coeffs=cf)
    out = torch.zeros((1, 256, 512), dtype=torch.int16, device=DEV)
    fz.stitch(t_tiles, out, coeffs=cf)
    fz.synchronize()
    assert np.array_equal(_png16_read(res / (RAW + ".png")), out.cpu().numpy().view(np.uint16)[0])
    fz.close()


def test_set_tile_validity_from_cpp():
    """SetTileValidity, then StitchDepthMaps / SolveDepthAll / SolveDepthBySmoothing from compiled
    C++ (tests/cpp/valid_link.cpp) against the binding on the same hand-filled maps."""
    _need_gpu()
    r = subprocess.run([LINK, "gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = {ln.split()[0]: ln.split()[1:] for ln in r.stdout.splitlines()
            if ln.split()[:1] and ln.split()[0] in ("STITCH", "FUSE", "PLAIN", "BADRANGE",
                                                    "SMOOTHING")}
    assert rows["BADRANGE"] == ["refused"] and rows["SMOOTHING"] == ["refused"]
    assert "pf_set_tile_validity" in r.stdout  # the library's message for the smoothing
    tw, th = 64, 62
    lay = PL.leres_layout(tw, th)
    i = np.arange(tw * th, dtype=np.int64)
    data = np.stack([np.float32(0.1) + np.float32(0.8)
                     * ((i * 37 + p * 11) % 101).astype(np.float32) / np.float32(101.0)
                     for p in range(lay.ntiles)]).astype(np.float32).reshape(lay.ntiles, th, tw)
    data[3, 10:40, 20:50] = np.nan
    data[7, 10:40, 20:50] = 0.0
    j = np.arange(64 * 32, dtype=np.int64)
    emap = (np.float32(0.2) + np.float32(0.6) * ((j * 37) % 101).astype(np.float32)
            / np.float32(101.0)).astype(np.float32).reshape(1, 32, 64)

    def acc(a):
        s = 0
        for v in a.reshape(-1).tolist():
            s = (s * 1315423911 + v) & 0xFFFFFFFFFFFFFFFF
        return str(s)

    fz = panofuse.Fuser(0)
    fz.set_tiles(lay)
    t = torch.from_numpy(data.reshape(1, -1)).to(DEV).contiguous()
    st = torch.zeros((1, 50, 100), dtype=torch.int16, device=DEV)
    fu = torch.zeros((1, 256, 512), dtype=torch.int16, device=DEV)
    fz.set_tile_validity(lo=0.0)
    fz.stitch(t, st)
    fz.fuse(torch.from_numpy(emap).to(DEV).contiguous(), t, fu, ZR)
    fz.synchronize()
    masked = st.cpu().numpy().view(np.uint16)[0].copy()
    assert rows["STITCH"] == ["100", "50", acc(masked)]
    assert rows["FUSE"] == ["512", "256", acc(fu.cpu().numpy().view(np.uint16)[0])]
    fz.set_tile_validity(None, None)
    fz.stitch(t, st)
    fz.synchronize()
    plain = st.cpu().numpy().view(np.uint16)[0]
    assert rows["PLAIN"] == ["100", "50", acc(plain)]
    assert not np.array_equal(plain, masked)
    fz.close()
