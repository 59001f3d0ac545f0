"""GPU end-to-end of the overlap-consistent registration on the command line and through the facade.

Mode 0 on a small folder (512x256 output, 128x64 baseline, the default table's 15 tiles at 128x124
as 16-bit PNGs, the pattern of tests/test_gpu_planar_cli.py): with --reg-consistent 1 the result
PNG is what register_consistent + fuse (or stitch) give through the binding, byte for byte, and the
"[consistent]" line carries the binding's pair counts and overlap rms, after <= before; the
combinations it has no form for are refused and write nothing; malformed values exit with status
2; without the flag no such line appears and the PNG is the default merge's.
tests/cpp/consist_link.cpp calls SolveDepthToDepthConsistent and TileOverlapStats from compiled
C++ against the binding on the same hand-filled maps."""
import os
import re
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import consist_ref as CR  # noqa: E402
import panofuse  # noqa: E402
import pf_layouts as PL  # noqa: E402
import pf_synth  # noqa: E402
import pyoracle as O  # noqa: E402
from test_gpu_disp_cli import _png16_read, _png16_write, _q16  # noqa: E402

PKG = os.path.dirname(os.path.dirname(panofuse.LIB_PATH))
MAIN = os.path.join(PKG, "bin", "panofuse_main")
LINK = os.path.join(PKG, "bin", "pf_consist_link")
ZR = PL.ZENITH_RANGE
DEV = "cuda:0"
RAW = "scene01_rgb"
TW, TH = 128, 124
ENV_SWITCHES = ("PF_REG_LOSS", "PF_TILE_VALID", "PF_TILE_DEPTH", "PF_TILE_MODEL", "PF_FUSION",
                "PF_REG_CONSISTENT", "PF_GLOBAL_ALIGN")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected on a host without a GPU")


def _tone(z, p):
    return ((0.8 + 0.05 * (p % 3)) * z.astype(np.float64) ** (1.1 - 0.05 * (p % 2)) + 0.03
            ).astype(np.float32)


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    _need_gpu()
    root = tmp_path_factory.mktemp("consist_cli")
    d = {k: root / k for k in ("rgb", "gt", "base", "tiles")}
    for p in d.values():
        p.mkdir()
    lay = PL.leres_layout(TW, TH)
    tiles, total = O.make_tiles(lay)
    seeds = pf_synth.seeds_for(1, 20261020 + 57)
    gt = pf_synth.scene_depth(seeds, 512, 256)[0].numpy()
    base = pf_synth.baseline_emap(seeds, 128, 64)[0].numpy()
    depth = O.warp_depth(gt, tiles, total, O.responses(pf_synth.responses(seeds, lay.ntiles)))
    for p, t in enumerate(tiles):  # per-tile tone curves: the neighbours disagree
        s = slice(t.offset, t.offset + t.width * t.height)
        depth[s] = _tone(depth[s], p)
    (d["rgb"] / (RAW + ".jpg")).write_bytes(b"\xff\xd8")  # only the name is used
    tq = _q16(depth).reshape(lay.ntiles, TH, TW).copy()
    bq = _q16(base).copy()
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
        env = {k: v for k, v in os.environ.items() if k not in ENV_SWITCHES}
        return subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=env), res

    t_emap = torch.from_numpy(bq.astype(np.float32) / np.float32(65535.0))[None].to(DEV)
    t_tiles = torch.from_numpy((tq.astype(np.float32) / np.float32(65535.0)).reshape(1, -1)).to(DEV)
    return run, lay, t_emap.contiguous(), t_tiles.contiguous()


def _binding(lay, t_emap, t_tiles, lam, fusion="laplacian"):
    """(result u16, pairs, pair samples, overlap rms before, after); lam None: the default merge."""
    fz = panofuse.Fuser(0)
    fz.set_tiles(lay)
    out = torch.zeros((1, 256, 512), dtype=torch.int16, device=DEV)
    cf = torch.zeros((1, lay.ntiles, 4), dtype=torch.float32, device=DEV)
    info = None
    if lam is None:
        fz.register(t_emap, t_tiles, ZR, apply=False, coeffs=cf)
    else:
        fz.register(t_emap, t_tiles, ZR, apply=False, coeffs=cf)
        before = CR.overlap_rms(fz.overlap_stats(t_tiles, ZR, coeffs=cf).cpu().numpy())
        fz.register_consistent(t_emap, t_tiles, ZR, lam=lam, apply=False, coeffs=cf)
        after = CR.overlap_rms(fz.overlap_stats(t_tiles, ZR, coeffs=cf).cpu().numpy())
        info = fz.overlap_pairs(ZR) + (before, after)
    if fusion == "stitch":
        fz.stitch(t_tiles, out, cf)
    else:
        fz.fuse(t_emap, t_tiles, out, ZR, cf)
    fz.synchronize()
    fz.close()
    return out.cpu().numpy().view(np.uint16)[0], info


@pytest.mark.parametrize("opts", [[], ["--fusion", "stitch"]])
def test_reg_consistent(folder, opts):
    run, lay, t_emap, t_tiles = folder
    r, res = run("consistent" + "_".join(o.strip("-") for o in opts), "--reg-consistent", "1", *opts)
    assert r.returncode == 0, r.stdout + r.stderr
    fusion = "stitch" if "stitch" in opts else "laplacian"
    want, (npairs, nsamp, before, after) = _binding(lay, t_emap, t_tiles, 1.0, fusion)
    got = _png16_read(res / (RAW + ".png"))
    assert np.array_equal(got, want)
    assert not np.array_equal(want, _binding(lay, t_emap, t_tiles, None, fusion)[0])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("[consistent]")]
    assert lines == [f"[consistent] lambda 1: {npairs} pairs, {nsamp} pair samples, overlap rms "
                     f"{before:.6g} -> {after:.6g}"], r.stdout
    assert after <= before and npairs > 0


def test_without_the_flag_nothing_changes(folder):
    run, lay, t_emap, t_tiles = folder
    r, res = run("plain")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "[consistent]" not in r.stdout
    assert np.array_equal(_png16_read(res / (RAW + ".png")),
                          _binding(lay, t_emap, t_tiles, None)[0])


@pytest.mark.parametrize("opts,setter", [
    (["--tile-valid", "0:1"], "pf_set_tile_validity"),
    (["--reg-loss", "huber:0.02"], "pf_set_register_loss"),
    (["--tile-depth", "planar"], "pf_set_tile_depth")])
def test_modes_are_refused_with_the_librarys_message(folder, opts, setter):
    run = folder[0]
    r, res = run("mode_" + opts[0].strip("-"), "--reg-consistent", "1", *opts)
    assert "pf_register_consistent" in r.stdout and setter in r.stdout, r.stdout + r.stderr
    assert "[consistent]" not in r.stdout and not (res / (RAW + ".png")).exists()


@pytest.mark.parametrize("opts", [["--tile-model", "disparity"], ["--global-align"]])
def test_other_combinations_are_refused_before_any_gpu_call(folder, opts):
    run = folder[0]
    for order in (["--reg-consistent", "1"] + opts, opts + ["--reg-consistent", "1"]):
        r, res = run("combo_" + re.sub(r"\W", "_", " ".join(order)), *order)
        assert r.returncode == 2, r.stdout + r.stderr
        assert r.stdout == ("--reg-consistent registers depth tiles by a linear solve: not with "
                            + " ".join(opts) + "\n")
        assert not (res / (RAW + ".png")).exists()


def test_bad_values_are_refused(folder):
    run = folder[0]
    for bad in ("-1", "abc", "1x", "nan", "inf", "-0.5", "1e999"):
        r, res = run("bad_" + re.sub(r"\W", "_", bad), "--reg-consistent", bad)
        assert r.returncode == 2, r.stdout + r.stderr
        assert r.stdout == f"bad --reg-consistent {bad} (want a finite LAMBDA >= 0)\n"
        assert not (res / (RAW + ".png")).exists()


def test_facade_from_cpp():
    """SolveDepthToDepthConsistent and TileOverlapStats from compiled C++
    (tests/cpp/consist_link.cpp) against the binding on the same hand-filled maps."""
    _need_gpu()
    r = subprocess.run([LINK, "gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = {}
    for ln in r.stdout.splitlines():
        w = ln.split()
        if w[:1] and w[0] in ("BADLAMBDA", "PLANAR", "CONS", "RAW", "FIT"):
            rows.setdefault(w[0], []).append(w[1:])
    assert rows["BADLAMBDA"] == [["refused"]] and rows["PLANAR"] == [["refused"]]
    assert "lambda" in r.stdout and "pf_set_tile_depth" in r.stdout

    tw, th = 64, 62
    lay = PL.leres_layout(tw, th)
    i = np.arange(tw * th, dtype=np.int64)
    data = np.stack([np.float32(0.1) + np.float32(0.8)
                     * ((i * 37 + p * 11) % 101).astype(np.float32) / np.float32(101.0)
                     for p in range(lay.ntiles)]).astype(np.float32)
    j = np.arange(64 * 32, dtype=np.int64)
    emap = (np.float32(0.2) + np.float32(0.6) * ((j * 37) % 101).astype(np.float32)
            / np.float32(101.0)).astype(np.float32).reshape(1, 32, 64)
    t_emap = torch.from_numpy(emap).to(DEV).contiguous()
    t = torch.from_numpy(data.reshape(1, -1)).to(DEV).contiguous()
    fz = panofuse.Fuser(0)
    fz.set_tiles(lay)
    cf = torch.zeros((1, lay.ntiles, 4), dtype=torch.float32, device=DEV)
    fz.register_consistent(t_emap, t, ZR, lam=1.0, apply=False, coeffs=cf)
    raw = fz.overlap_stats(t, ZR).cpu().numpy()[0]
    fit = fz.overlap_stats(t, ZR, coeffs=cf).cpu().numpy()[0]
    pairs, _ = fz.overlap_table(ZR)
    fz.synchronize()
    pairs = pairs.cpu().numpy()
    fz.close()
    cons = np.array([[float(v) for v in w[1:]] for w in rows["CONS"]], np.float32)
    assert [int(w[0]) for w in rows["CONS"]] == list(range(lay.ntiles))
    assert np.array_equal(cons.view(np.uint32), cf.cpu().numpy()[0].view(np.uint32))
    for tag, want in (("RAW", raw), ("FIT", fit)):
        got = np.array([[float(v) for v in w] for w in rows[tag]], np.float64)
        assert np.array_equal(got[:, :2], pairs[:, :2])
        assert np.array_equal(got[:, 2:].view(np.uint64), want.view(np.uint64)), tag
