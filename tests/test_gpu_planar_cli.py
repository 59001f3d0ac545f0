"""GPU end-to-end of planar-depth tiles on the command line and through the facade.

Mode 0 on a C1-sized folder (512x256 output, 128x64 baseline, the default table's 15 tiles at
256x247 as 16-bit PNGs, the pattern of tests/test_gpu_robust_cli.py): with --tile-depth planar the
result PNG equals the binding's output in planar mode byte for byte and the "[tile-depth]" line is
printed, for both tile models and for --fusion stitch; without the flag (and with --tile-depth
ray) the PNG is the default merge's and no such line appears; a bad value exits with status 2.
tests/cpp/planar_link.cpp calls SetTileDepth from compiled C++ against the binding on the same
hand-filled maps."""
import os
import re
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import panofuse  # noqa: E402
import pf_layouts as PL  # noqa: E402
import pf_synth  # noqa: E402
import planar_ref as P  # noqa: E402
import pyoracle as O  # noqa: E402
from test_gpu_disp_cli import _png16_read, _png16_write, _q16  # noqa: E402

PKG = os.path.dirname(os.path.dirname(panofuse.LIB_PATH))
MAIN = os.path.join(PKG, "bin", "panofuse_main")
LINK = os.path.join(PKG, "bin", "pf_planar_link")
ZR = PL.ZENITH_RANGE
DEV = "cuda:0"
RAW = "scene01_rgb"
TW, TH = 256, 247


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected on a host without a GPU")


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    _need_gpu()
    root = tmp_path_factory.mktemp("planar_cli")
    d = {k: root / k for k in ("rgb", "gt", "base", "tiles")}
    for p in d.values():
        p.mkdir()
    lay = PL.leres_layout(TW, TH)
    tiles, total = O.make_tiles(lay)
    seeds = pf_synth.seeds_for(1, 20261020 + 56)
    gt = pf_synth.scene_depth(seeds, 512, 256)[0].numpy()
    base = pf_synth.baseline_emap(seeds, 128, 64)[0].numpy()
    depth = O.warp_depth(gt, tiles, total, O.responses(pf_synth.responses(seeds, lay.ntiles)))
    kfs = P.layout_kf(lay)
    for p, t in enumerate(tiles):  # planar depth: the ray distance over the factor
        s = slice(t.offset, t.offset + t.width * t.height)
        depth[s] = depth[s] / kfs[p].reshape(-1)
    (d["rgb"] / (RAW + ".jpg")).write_bytes(b"\xff\xd8")  # only the name is used
    tq = _q16(depth).reshape(lay.ntiles, TH, TW).copy()
    bq = _q16(base).copy()
    _png16_write(d["gt"] / (RAW.replace("_rgb", "_depth") + ".png"), _q16(gt))
    _png16_write(d["base"] / (RAW + ".depth.png"), bq)
    names = PL.tile_names(lay)
    for t in range(lay.ntiles):
        _png16_write(d["tiles"] / f"{RAW}.{names[t]}.png", tq[t])

    def run(tag, *opts, env_extra=None):
        res = root / tag / "result_hohonet"
        res.mkdir(parents=True)
        cmd = [MAIN, "0", str(d["rgb"]), str(d["gt"]), str(d["base"]), str(res), "--tiles",
               str(d["tiles"]), "--ext", "png", "--width", "512"] + list(opts)
        env = {k: v for k, v in os.environ.items()
               if k not in ("PF_REG_LOSS", "PF_TILE_VALID", "PF_TILE_DEPTH", "PF_TILE_MODEL",
                            "PF_FUSION")}
        env.update(env_extra or {})
        return subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=env), res

    t_emap = torch.from_numpy(bq.astype(np.float32) / np.float32(65535.0))[None].to(DEV)
    t_tiles = torch.from_numpy((tq.astype(np.float32) / np.float32(65535.0)).reshape(1, -1)).to(DEV)
    return run, lay, t_emap.contiguous(), t_tiles.contiguous(), float(max(k.max() for k in kfs))


def _binding(lay, t_emap, t_tiles, depth, model="depth", fusion="laplacian"):
    fz = panofuse.Fuser(0)
    fz.set_tiles(lay)
    fz.set_tile_depth(depth)
    out = torch.zeros((1, 256, 512), dtype=torch.int16, device=DEV)
    if fusion == "stitch":
        copy = t_tiles.clone()
        cf = torch.zeros((1, lay.ntiles, 4), dtype=torch.float32, device=DEV)
        if depth == "planar":
            fz.register(t_emap, copy, ZR, apply=True, coeffs=cf)
            fz.stitch(copy, out)
        else:
            fz.register(t_emap, copy, ZR, apply=False, coeffs=cf)
            fz.stitch(copy, out, cf)
    elif model == "disparity":
        fz.merge_disparity(t_emap, t_tiles, out, ZR)
    else:
        fz.merge(t_emap, t_tiles, out, ZR)
    fz.synchronize()
    fz.close()
    return out.cpu().numpy().view(np.uint16)[0]


@pytest.mark.parametrize("how,opts", [
    ("flag", []), ("env", []), ("flag", ["--tile-model", "disparity"]),
    ("flag", ["--fusion", "stitch"])])
def test_tile_depth_planar(folder, how, opts):
    run, lay, t_emap, t_tiles, kmax = folder
    tag = "planar_" + how + "_".join(o.strip("-") for o in opts)
    if how == "flag":
        r, res = run(tag, "--tile-depth", "planar", *opts)
    else:
        r, res = run(tag, *opts, env_extra={"PF_TILE_DEPTH": "planar"})
    assert r.returncode == 0, r.stdout + r.stderr
    got = _png16_read(res / (RAW + ".png"))
    model = "disparity" if "disparity" in opts else "depth"
    fusion = "stitch" if "stitch" in opts else "laplacian"
    want = _binding(lay, t_emap, t_tiles, "planar", model, fusion)
    assert np.array_equal(got, want)
    assert not np.array_equal(want, _binding(lay, t_emap, t_tiles, "ray", model, fusion))
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("[tile-depth]")]
    assert lines == [f"[tile-depth] planar: ray factor up to {kmax:.3f} over {lay.ntiles} tiles"], \
        r.stdout


def test_without_the_flag_nothing_changes(folder):
    run, lay, t_emap, t_tiles, _ = folder
    r, res = run("plain")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "[tile-depth]" not in r.stdout
    plain = _binding(lay, t_emap, t_tiles, None)
    assert np.array_equal(_png16_read(res / (RAW + ".png")), plain)
    r2, res2 = run("ray", "--tile-depth", "ray")
    assert r2.returncode == 0, r2.stdout + r2.stderr
    assert np.array_equal(_png16_read(res2 / (RAW + ".png")), plain)

    def stable(text, res_dir):  # without this run's folder and the timings' digits
        return re.sub(r"(@|time_Reg:|time_Laplacian:)\d+", r"\1", text.replace(str(res_dir), "RES"))
    assert stable(r.stdout, res) == stable(r2.stdout, res2)


def test_bad_values_are_refused(folder):
    run = folder[0]
    for bad in ("plane", "Planar", "1", "planar,ray"):
        r, res = run("bad_" + re.sub(r"\W", "_", bad), "--tile-depth", bad)
        assert r.returncode == 2, r.stdout + r.stderr
        assert r.stdout == f"bad --tile-depth {bad} (want planar or ray)\n"
        assert not (res / (RAW + ".png")).exists()
    r, res = run("bad_env", env_extra={"PF_TILE_DEPTH": "plane"})
    assert "bad PF_TILE_DEPTH plane" in r.stdout and not (res / (RAW + ".png")).exists()


def test_set_tile_depth_from_cpp():
    """SetTileDepth, then SolveDepthToDepth / SolveDisparityToDepth from compiled C++
    (tests/cpp/planar_link.cpp) against the binding on the same hand-filled maps."""
    _need_gpu()
    r = subprocess.run([LINK, "gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    tags = ("BADKIND", "PLANAR", "PLANARDISP", "RAY", "JOINT")
    rows = {}
    for ln in r.stdout.splitlines():
        w = ln.split()
        if w[:1] and w[0] in tags:
            rows.setdefault(w[0], []).append(w[1:])
    assert rows["BADKIND"] == [["refused"]]
    assert rows["JOINT"][0] == ["refused"] and len(rows["JOINT"]) == 2
    assert "[SetTileDepth]" in r.stdout and "pf_set_tile_depth" in r.stdout

    tw, th = 64, 62
    full = PL.leres_layout(tw, th)
    i = np.arange(tw * th, dtype=np.int64)
    data = np.stack([np.float32(0.1) + np.float32(0.8)
                     * ((i * 37 + p * 11) % 101).astype(np.float32) / np.float32(101.0)
                     for p in range(full.ntiles)]).astype(np.float32)
    j = np.arange(64 * 32, dtype=np.int64)
    emap = (np.float32(0.2) + np.float32(0.6) * ((j * 37) % 101).astype(np.float32)
            / np.float32(101.0)).astype(np.float32).reshape(1, 32, 64)
    t_emap = torch.from_numpy(emap).to(DEV).contiguous()
    ids = [2]
    lay = PL.Layout("sub", full.fovs[ids].copy(), full.ranges[ids].copy(),
                    full.tile_w[ids].copy(), full.tile_h[ids].copy())
    t = torch.from_numpy(data[ids].reshape(1, -1)).to(DEV).contiguous()

    def f32_row(words):
        return np.array([float(w) for w in words], np.float32)

    fz = panofuse.Fuser(0)
    fz.set_tiles(lay)
    cf = torch.zeros((1, 1, 4), dtype=torch.float32, device=DEV)
    got = {}
    for tag, depth, call in (("PLANAR", "planar", fz.register), ("RAY", "ray", fz.register),
                             ("PLANARDISP", "planar", fz.register_disparity)):
        fz.set_tile_depth(depth)
        call(t_emap, t, ZR, apply=False, coeffs=cf)
        fz.synchronize()
        got[tag] = cf.cpu().numpy()[0, 0].copy()
    fz.close()
    for tag in ("PLANAR", "RAY", "PLANARDISP"):
        assert np.array_equal(f32_row(rows[tag][0]), got[tag]), (tag, rows[tag], got[tag])
    assert not np.array_equal(got["PLANAR"], got["RAY"])
