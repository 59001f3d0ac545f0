"""GPU end-to-end of the mode-0 switches --save-stitch, --check-laplacian and --fusion: one tiny
folder (512x256 output, 128x64 baseline, LeReS' 15 windows with 256x247 tiles, the fixture of
tests/test_gpu_global_cli.py), every run held to the binding on the pixels the files decode to;
and the facade's StitchDepthMaps / CheckLaplacian called from compiled C++
(tests/cpp/stitch_link.cpp), held to the binding and to the CPU restatement (tests/stitch_ref.py).
"""
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
import stitch_ref as S  # noqa: E402
from test_gpu_global_cli import (MAIN, MYPI, PKG, _cround, _fill, _png16_read,  # noqa: E402
                                 _png16_write, _q16)

LINK = os.path.join(PKG, "bin", "pf_stitch_link")
ZR = PL.ZENITH_RANGE
DEV = "cuda:0"
RAW = "scene01_rgb"
SWITCHES = ("PF_FUSION", "PF_SAVE_STITCH", "PF_CHECK_LAPLACIAN", "PF_GLOBAL_ALIGN")


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected on a host without a GPU")
    root = tmp_path_factory.mktemp("stitch_cli")
    d = {k: root / k for k in ("rgb", "gt", "base", "tiles")}
    for p in d.values():
        p.mkdir()
    tw, th = 256, 247
    lay = PL.leres_layout(tw, th)
    tiles, total = O.make_tiles(lay)
    seeds = pf_synth.seeds_for(1, 20261020 + 5)
    gt = pf_synth.scene_depth(seeds, 512, 256)[0].numpy()
    base = pf_synth.baseline_emap(seeds, 128, 64)[0].numpy()
    depth = O.warp_depth(gt, tiles, total, O.responses(pf_synth.responses(seeds, lay.ntiles)))
    (d["rgb"] / (RAW + ".jpg")).write_bytes(b"\xff\xd8")  # only the name is used
    gq, bq, tq = _q16(gt), _q16(base), _q16(depth)
    _png16_write(d["gt"] / (RAW.replace("_rgb", "_depth") + ".png"), gq)
    _png16_write(d["base"] / (RAW + ".depth.png"), bq)  # hohonet naming (Main.cpp:512-516)
    for t in range(lay.ntiles):
        f = [_cround(float(v) / MYPI * 180.0) for v in lay.fovs[t]]
        _png16_write(d["tiles"] / f"{RAW}.{f[0]}_{f[1]}_{f[2]}_{f[3]}.png",
                     tq[t * tw * th:(t + 1) * tw * th].reshape(th, tw))

    # the binding on the pixels the files decode to
    fz = panofuse.Fuser(0)
    fz.set_tiles(lay)
    emap = torch.from_numpy(bq.astype(np.float32) / np.float32(65535.0))[None].to(DEV).contiguous()
    tl = torch.from_numpy(tq.astype(np.float32) / np.float32(65535.0))[None].to(DEV).contiguous()
    cf = torch.zeros((1, lay.ntiles, 4), dtype=torch.float32, device=DEV)
    fz.register(emap, tl, ZR, degree=3, apply=False, coeffs=cf)
    outs = {k: torch.zeros((1, 256, 512), dtype=torch.int16, device=DEV)
            for k in ("fuse", "stitch", "smoothing")}
    fz.fuse(emap, tl, outs["fuse"], ZR, coeffs=cf)
    fz.stitch(tl, outs["stitch"], coeffs=cf)
    fz.solve_smoothing(tl, outs["smoothing"], ZR, coeffs=cf)
    err = fz.fuse_check(emap, tl, ZR, 512, coeffs=cf)
    fz.synchronize()
    ref = {k: v.cpu().numpy().view(np.uint16)[0] for k, v in outs.items()}
    ref["err"] = err.cpu().numpy()
    fz.close()

    def run(name, *flags):
        res = root / name / "result_hohonet"
        res.mkdir(parents=True)
        cmd = [MAIN, "0", str(d["rgb"]), str(d["gt"]), str(d["base"]), str(res), "--tiles",
               str(d["tiles"]), "--ext", "png", "--width", "512", *flags]
        env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=env)
        return r, res
    return run, ref


@pytest.fixture(scope="module")
def plain(folder):
    run, ref = folder
    r, res = run("plain")
    assert r.returncode == 0, r.stdout + r.stderr
    return r, res


def test_default_run_is_the_fusion(folder, plain):
    run, ref = folder
    r, res = plain
    assert np.array_equal(_png16_read(res / (RAW + ".png")), ref["fuse"])
    assert "check Laplacian" not in r.stdout
    assert not (res / (RAW + ".png.pmap.png")).exists()
    assert not np.array_equal(ref["fuse"], ref["stitch"])
    assert not np.array_equal(ref["smoothing"], ref["stitch"])


def test_save_stitch_and_check_laplacian(folder, plain):
    run, ref = folder
    r, res = run("diag", "--save-stitch", "--check-laplacian")
    assert r.returncode == 0, r.stdout + r.stderr
    assert np.array_equal(_png16_read(res / (RAW + ".png.pmap.png")), ref["stitch"])
    # the files the plain run writes are unchanged, byte for byte
    _, res0 = plain
    names = sorted(p.name for p in res0.iterdir())
    assert sorted(p.name for p in res.iterdir()) == sorted(names + [RAW + ".png.pmap.png"])
    for n in names:
        assert (res / n).read_bytes() == (res0 / n).read_bytes(), n
    lines = [ln for ln in r.stdout.splitlines() if "check Laplacian err:" in ln]
    assert len(lines) == 1 and lines[0].startswith("[SolveDepthAll] check Laplacian err:"), r.stdout
    got = float(lines[0].split("err:")[1])
    want = float(ref["err"][-1])
    print(f"check Laplacian: printed {lines[0]!r}, fuse_check {ref['err']}")
    assert np.isfinite(want) and want > 0
    assert got == float(f"{want:.6g}")


def test_fusion_stitch(folder):
    run, ref = folder
    r, res = run("stitch", "--fusion", "stitch")
    assert r.returncode == 0, r.stdout + r.stderr
    assert np.array_equal(_png16_read(res / (RAW + ".png")), ref["stitch"])


def test_fusion_smoothing(folder):
    run, ref = folder
    r, res = run("smoothing", "--fusion", "smoothing")
    assert r.returncode == 0, r.stdout + r.stderr
    assert np.array_equal(_png16_read(res / (RAW + ".png")), ref["smoothing"])


def test_facade_calls_from_cpp():
    """StitchDepthMaps and CheckLaplacian called from compiled C++ (tests/cpp/stitch_link.cpp)
    against the binding and the restatement on the same hand-filled maps."""
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected on a host without a GPU")
    r = subprocess.run([LINK, "gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [ln.split() for ln in r.stdout.splitlines() if ln.startswith(("STITCH", "ERR"))]
    tw, th = 64, 62
    lay = PL.leres_layout(tw, th)
    tiles = O.make_tiles(lay)[0]
    i = np.arange(tw * th, dtype=np.int64)
    data = np.concatenate([(((i * 37 + p * 11) % 101).astype(np.float32) / np.float32(101.0))
                           for p in range(lay.ntiles)]).astype(np.float32)
    fz = panofuse.Fuser(0)
    fz.set_tiles(lay)
    t = torch.from_numpy(data)[None].to(DEV).contiguous()
    for row, (w, h) in zip(rows[:2], [(100, 50), (101, 51)]):
        out = torch.zeros((1, h, w), dtype=torch.int16, device=DEV)
        fz.stitch(t, out)
        fz.synchronize()
        want = out.cpu().numpy().view(np.uint16)[0]
        assert np.array_equal(want, S.stitch(tiles, data, w, h))
        acc = 0
        for v in want.reshape(-1).tolist():
            acc = (acc * 1315423911 + v) & 0xFFFFFFFFFFFFFFFF
        assert row == ["STITCH", str(w), str(h), str(acc)]
    emap = torch.from_numpy(_fill(64, 32, 0.6, 0.2))[None].to(DEV).contiguous()
    err = fz.fuse_check(emap, t, ZR, 512).cpu().numpy()
    fz.close()
    assert rows[2][:2] == ["ERR", str(err.size)] and err.size == 3
    got = np.array([np.float32(v) for v in rows[2][2:]], np.float32)
    assert np.array_equal(got.view(np.uint32), err.view(np.uint32))
    assert np.isfinite(err).all() and (err > 0).all()


def test_check_laplacian_needs_the_fusion(folder):
    run, ref = folder
    r, res = run("refused", "--check-laplacian", "--fusion", "stitch")
    assert r.returncode != 0
    assert "--check-laplacian needs --fusion laplacian" in r.stdout
    assert not any(res.iterdir())
    r, _ = run("badfusion", "--fusion", "median")
    assert r.returncode != 0 and "bad --fusion" in r.stdout
