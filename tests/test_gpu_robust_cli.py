"""GPU end-to-end of the robust registration loss on the command line and through the facade.

Mode 0 on a C1-sized folder (512x256 output, 128x64 baseline, the default table's 15 tiles at
256x247 as 16-bit PNGs, the pattern of tests/test_gpu_mask_cli.py): with --reg-loss huber:0.02 the
result PNG equals the binding's output under the same loss and one "[robust]" line per tile is
printed; without the flag no "[robust]" line is printed and the PNG is the default merge's.
--global-align together with the flag is refused.  tests/cpp/robust_link.cpp calls
SetRegistrationLoss from compiled C++ against the binding on the same hand-filled maps."""
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
import pyoracle as O  # noqa: E402
from test_gpu_disp_cli import _png16_read, _png16_write, _q16  # noqa: E402

PKG = os.path.dirname(os.path.dirname(panofuse.LIB_PATH))
MAIN = os.path.join(PKG, "bin", "panofuse_main")
LINK = os.path.join(PKG, "bin", "pf_robust_link")
ZR = PL.ZENITH_RANGE
DEV = "cuda:0"
RAW = "scene01_rgb"
TW, TH = 256, 247
TERMINATION = ("no convergence", "function tolerance", "parameter tolerance",
               "gradient tolerance", "minimum trust-region radius", "failure")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected on a host without a GPU")


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    _need_gpu()
    root = tmp_path_factory.mktemp("robust_cli")
    d = {k: root / k for k in ("rgb", "gt", "base", "tiles")}
    for p in d.values():
        p.mkdir()
    lay = PL.leres_layout(TW, TH)
    tiles, total = O.make_tiles(lay)
    seeds = pf_synth.seeds_for(1, 20261020 + 55)
    gt = pf_synth.scene_depth(seeds, 512, 256)[0].numpy()
    base = pf_synth.baseline_emap(seeds, 128, 64)[0].numpy()
    depth = O.warp_depth(gt, tiles, total, O.responses(pf_synth.responses(seeds, lay.ntiles)))
    (d["rgb"] / (RAW + ".jpg")).write_bytes(b"\xff\xd8")  # only the name is used
    tq = _q16(depth).reshape(lay.ntiles, TH, TW).copy()
    bq = _q16(base).copy()
    rng = np.random.default_rng(9)  # 10 % of the baseline replaced: outliers in y
    hit = rng.random(bq.shape) < 0.10
    bq[hit] = rng.integers(1, 65535, int(hit.sum())).astype(bq.dtype)
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
        env = {k: v for k, v in os.environ.items() if k not in ("PF_REG_LOSS", "PF_TILE_VALID")}
        env.update(env_extra or {})
        return subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=env), res

    t_emap = torch.from_numpy(bq.astype(np.float32) / np.float32(65535.0))[None].to(DEV)
    t_tiles = torch.from_numpy((tq.astype(np.float32) / np.float32(65535.0)).reshape(1, -1)).to(DEV)
    return run, lay, t_emap.contiguous(), t_tiles.contiguous()


def _binding(lay, t_emap, t_tiles, loss):
    fz = panofuse.Fuser(0)
    fz.set_tiles(lay)
    if loss:
        fz.set_register_loss(*loss)
    out = torch.zeros((1, 256, 512), dtype=torch.int16, device=DEV)
    sm = torch.zeros((1, lay.ntiles, 6), dtype=torch.float64, device=DEV)
    fz.merge(t_emap, t_tiles, out, ZR)
    if loss:
        fz.register(t_emap, t_tiles, ZR, apply=False, summary=sm)
    fz.synchronize()
    fz.close()
    return out.cpu().numpy().view(np.uint16)[0], sm.cpu().numpy()[0]


@pytest.mark.parametrize("how", ["flag", "env"])
def test_reg_loss_flag(folder, how):
    run, lay, t_emap, t_tiles = folder
    if how == "flag":
        r, res = run("huber_flag", "--reg-loss", "huber:0.02")
    else:
        r, res = run("huber_env", env_extra={"PF_REG_LOSS": "huber:0.02"})
    assert r.returncode == 0, r.stdout + r.stderr
    got = _png16_read(res / (RAW + ".png"))
    want, sm = _binding(lay, t_emap, t_tiles, ("huber", 0.02))
    assert np.array_equal(got, want)
    plain, _ = _binding(lay, t_emap, t_tiles, None)
    assert not np.array_equal(want, plain)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("[robust]")]
    assert len(lines) == lay.ntiles, r.stdout
    pat = re.compile(r"\[robust\] tile (\d+): (\d+) of (\d+) samples beyond a=0\.02, cost (\S+) -> "
                     r"(\S+), (\d+) iterations, (.+)$")
    for p, ln in enumerate(lines):
        m = pat.match(ln)
        assert m, ln
        assert int(m.group(1)) == p
        assert int(m.group(2)) == int(sm[p, 4] - sm[p, 5]) and int(m.group(3)) == int(sm[p, 4])
        assert 0 < int(m.group(2)) < int(m.group(3))
        assert abs(float(m.group(4)) - sm[p, 0]) <= 1e-5 * sm[p, 0]  # six printed digits
        assert abs(float(m.group(5)) - sm[p, 1]) <= 1e-5 * sm[p, 1]
        assert int(m.group(6)) == int(sm[p, 2]) and m.group(7) == TERMINATION[int(sm[p, 3])]


def test_without_the_flag_nothing_changes(folder):
    run, lay, t_emap, t_tiles = folder
    r, res = run("plain")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "[robust]" not in r.stdout
    plain, _ = _binding(lay, t_emap, t_tiles, None)
    assert np.array_equal(_png16_read(res / (RAW + ".png")), plain)


def test_bad_values_and_global_align_are_refused(folder):
    run = folder[0]
    for bad in ("huber", "huber:0", "cauchy:0.1", "softl1:x", "huber:-1", "huber:inf"):
        r, res = run("bad_" + re.sub(r"\W", "_", bad), "--reg-loss", bad)
        assert r.returncode == 2 and "bad --reg-loss" in r.stdout, r.stdout + r.stderr
        assert not (res / (RAW + ".png")).exists()
    r, res = run("global", "--reg-loss", "huber:0.02", "--global-align")
    assert "pf_set_register_loss" in r.stdout and "pf_register_global" in r.stdout, \
        r.stdout + r.stderr
    assert not (res / (RAW + ".png")).exists()


def test_set_registration_loss_from_cpp():
    """SetRegistrationLoss, then SolveDepthToDepth / SolveDepthToDepth2 from compiled C++
    (tests/cpp/robust_link.cpp) against the binding on the same hand-filled maps."""
    _need_gpu()
    r = subprocess.run([LINK, "gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    tags = ("BADLOSS", "HUBER", "SOFTL1", "PLAIN", "JOINT", "GLOBAL")
    rows = {}
    for ln in r.stdout.splitlines():
        w = ln.split()
        if w[:1] and w[0] in tags:
            rows.setdefault(w[0], []).append(w[1:])
    assert rows["BADLOSS"] == [["refused"]] and rows["GLOBAL"] == [["refused"]]
    assert rows["JOINT"][0] == ["refused"] and len(rows["JOINT"]) == 2
    assert "[SetRegistrationLoss]" in r.stdout
    assert r.stdout.count("pf_set_register_loss") >= 2  # the library's message, joint and global

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

    def sub(ids):
        lay = PL.Layout("sub", full.fovs[ids].copy(), full.ranges[ids].copy(),
                        full.tile_w[ids].copy(), full.tile_h[ids].copy())
        return lay, torch.from_numpy(data[ids].reshape(1, -1)).to(DEV).contiguous()

    def f32_row(words):
        return np.array([float(w) for w in words], np.float32)

    fz = panofuse.Fuser(0)
    lay, t = sub([2])
    fz.set_tiles(lay)
    cf = torch.zeros((1, 1, 4), dtype=torch.float32, device=DEV)
    got = {}
    for tag, loss in (("HUBER", ("huber", 0.02)), ("SOFTL1", ("softl1", 0.02))):
        fz.set_register_loss(*loss)
        fz.register(t_emap, t, ZR, apply=False, coeffs=cf)
        fz.synchronize()
        got[tag] = cf.cpu().numpy()[0, 0].copy()
    fz.set_register_loss(None)
    cj = torch.zeros((1, 4), dtype=torch.float32, device=DEV)
    fz.register_joint(t_emap, t, ZR, [0], coeffs=cj)
    fz.synchronize()
    got["PLAIN"] = cj.cpu().numpy()[0].copy()
    lay2, t2 = sub([2, 3])
    fz.set_tiles(lay2)
    fz.register_joint(t_emap, t2, ZR, [0, 1], coeffs=cj)
    fz.synchronize()
    got["JOINT"] = cj.cpu().numpy()[0].copy()
    fz.close()
    for tag in ("HUBER", "SOFTL1", "PLAIN"):
        assert np.array_equal(f32_row(rows[tag][0]), got[tag]), (tag, rows[tag], got[tag])
    assert np.array_equal(f32_row(rows["JOINT"][1]), got["JOINT"])
    assert not np.array_equal(got["HUBER"], got["PLAIN"])
    assert not np.array_equal(got["HUBER"], got["SOFTL1"])
