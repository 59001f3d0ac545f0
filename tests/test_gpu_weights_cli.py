"""GPU end-to-end of the per-pixel tile weights on the command line and through the facade.

Mode 0 on a C1-sized folder (512x256 output, 128x64 baseline, the default table's 15 tiles at
256x247 as 16-bit PNGs, the pattern of tests/test_gpu_planar_cli.py): with --tile-weights tent, and
with files:.w.pfm over a fixed-seed smooth field, the result PNG equals the binding's
merge_weighted byte for byte and the "[weights]" lines carry register_weighted's summary; a
weight file of another size is refused by name; the flag next to an option it cannot go with is
refused before any GPU call (tests/test_weights_sanitized.py runs every such pair without a GPU);
without the flag the run writes the files and lines it always wrote.
tests/cpp/weights_link.cpp calls SetTileWeights + MergeDepthMaps from compiled C++ on the same
folder."""
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
import weight_ref as WR  # noqa: E402
from test_gpu_disp_cli import _png16_read, _png16_write, _q16  # noqa: E402
from test_weights_sanitized import ENV_DROP  # noqa: E402

PKG = os.path.dirname(os.path.dirname(panofuse.LIB_PATH))
MAIN = os.path.join(PKG, "bin", "panofuse_main")
LINK = os.path.join(PKG, "bin", "pf_weights_link")
ZR = PL.ZENITH_RANGE
DEV = "cuda:0"
RAW = "scene01_rgb"
TW, TH = 256, 247
SUFFIX = ".w.pfm"


def _pfm_write(path, a):
    """One-channel little-endian PFM, rows in the order the map loader reads them."""
    h, w = a.shape
    with open(path, "wb") as f:
        f.write(f"Pf\n{w} {h}\n-1.0\n".encode())
        f.write(np.ascontiguousarray(a, "<f4").tobytes())


def _field(lay):
    """A fixed-seed smooth weight set in [0.1, 1] with an exact-zero rectangle in tile 0 and odd
    values (NaN, negative, +inf) in tile 1: float32 [ntiles][TH][TW]."""
    rs = np.random.RandomState(20261021)
    g = 0.1 + 0.9 * rs.rand(lay.ntiles, 8, 8)
    ys, xs = np.linspace(0, 7, TH), np.linspace(0, 7, TW)
    y0, x0 = np.minimum(ys.astype(int), 6), np.minimum(xs.astype(int), 6)
    fy, fx = (ys - y0)[None, :, None], (xs - x0)[None, None, :]
    v = ((1 - fy) * (1 - fx) * g[:, y0][:, :, x0] + (1 - fy) * fx * g[:, y0][:, :, x0 + 1]
         + fy * (1 - fx) * g[:, y0 + 1][:, :, x0] + fy * fx * g[:, y0 + 1][:, :, x0 + 1])
    w = v.astype(np.float32)
    w[0, 100:, 100:180] = 0.0
    w[1, 50:60, 50:60] = np.nan
    w[1, 60:70, 50:60] = -1.0
    w[1, 70:80, 50:60] = np.inf
    return w


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected on a host without a GPU")
    root = tmp_path_factory.mktemp("weights_cli")
    d = {k: root / k for k in ("rgb", "gt", "base", "tiles", "badtiles")}
    for p in d.values():
        p.mkdir()
    lay = PL.leres_layout(TW, TH)
    tiles, total = O.make_tiles(lay)
    seeds = pf_synth.seeds_for(1, 20261020 + 57)
    gt = pf_synth.scene_depth(seeds, 512, 256)[0].numpy()
    base = pf_synth.baseline_emap(seeds, 128, 64)[0].numpy()
    depth = O.warp_depth(gt, tiles, total, O.responses(pf_synth.responses(seeds, lay.ntiles)))
    (d["rgb"] / (RAW + ".jpg")).write_bytes(b"\xff\xd8")  # only the name is used
    tq = _q16(depth).reshape(lay.ntiles, TH, TW).copy()
    bq = _q16(base).copy()
    _png16_write(d["gt"] / (RAW.replace("_rgb", "_depth") + ".png"), _q16(gt))
    _png16_write(d["base"] / (RAW + ".depth.png"), bq)
    names = PL.tile_names(lay)
    field = _field(lay)
    for t in range(lay.ntiles):
        for key in ("tiles", "badtiles"):
            _png16_write(d[key] / f"{RAW}.{names[t]}.png", tq[t])
        _pfm_write(d["tiles"] / f"{RAW}.{names[t]}.png{SUFFIX}", field[t])
        # tile 3's weight map of the other folder is transposed: 247 x 256
        _pfm_write(d["badtiles"] / f"{RAW}.{names[t]}.png{SUFFIX}",
                   field[t].T if t == 3 else field[t])

    def run(tag, *opts, env_extra=None, tiles_dir="tiles"):
        res = root / tag / "result_hohonet"
        res.mkdir(parents=True)
        cmd = [MAIN, "0", str(d["rgb"]), str(d["gt"]), str(d["base"]), str(res), "--tiles",
               str(d[tiles_dir]), "--ext", "png", "--width", "512"] + list(opts)
        env = {k: v for k, v in os.environ.items() if k not in ENV_DROP}
        env.update(env_extra or {})
        return subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=env), res

    t_emap = torch.from_numpy(bq.astype(np.float32) / np.float32(65535.0))[None].to(DEV)
    t_tiles = torch.from_numpy((tq.astype(np.float32) / np.float32(65535.0)).reshape(1, -1)).to(DEV)
    files = {"base": str(d["base"] / (RAW + ".depth.png")),
             "tiles": [str(d["tiles"] / f"{RAW}.{names[t]}.png") for t in range(lay.ntiles)]}
    return run, lay, t_emap.contiguous(), t_tiles.contiguous(), field, files


def _binding(lay, t_emap, t_tiles, weights):
    """(u16 result, summary [ntiles][2]) of merge_weighted / register_weighted; weights None: the
    plain merge."""
    fz = panofuse.Fuser(0)
    fz.set_tiles(lay)
    out = torch.zeros((1, 256, 512), dtype=torch.int16, device=DEV)
    sm = torch.zeros((1, lay.ntiles, 2), dtype=torch.float64, device=DEV)
    if weights is None:
        fz.merge(t_emap, t_tiles, out, ZR)
    else:
        w = fz.tent_weights() if isinstance(weights, str) else \
            torch.from_numpy(np.ascontiguousarray(weights).reshape(-1)).to(DEV)
        fz.merge_weighted(t_emap, t_tiles, w, out, ZR)
        fz.register_weighted(t_emap, t_tiles, w, ZR, apply=False, summary=sm)
    fz.synchronize()
    fz.close()
    return out.cpu().numpy().view(np.uint16)[0], sm.cpu().numpy()[0]


def _weights_lines(stdout):
    return [ln for ln in stdout.splitlines() if ln.startswith("[weights]")]


def _check_lines(lines, sm, lay):
    assert len(lines) == lay.ntiles
    for p, ln in enumerate(lines):
        m = re.fullmatch(r"\[weights\] tile (\d+): (\d+) of (\d+) samples used, sum w (\S+)", ln)
        assert m, ln
        assert (int(m.group(1)), int(m.group(2))) == (p, int(sm[p, 0])), ln
        assert int(m.group(3)) >= int(m.group(2)) > 0
        assert m.group(4) == "%.6g" % sm[p, 1], ln


@pytest.mark.parametrize("how", ["flag", "env"])
@pytest.mark.parametrize("kind", ["tent", "files"])
def test_tile_weights(folder, kind, how):
    run, lay, t_emap, t_tiles, field, _ = folder
    value = "tent" if kind == "tent" else "files:" + SUFFIX
    if how == "flag":
        r, res = run(f"{kind}_flag", "--tile-weights", value)
    else:
        r, res = run(f"{kind}_env", env_extra={"PF_TILE_WEIGHTS": value})
    assert r.returncode == 0, r.stdout + r.stderr
    want, sm = _binding(lay, t_emap, t_tiles, "tent" if kind == "tent" else field)
    assert np.array_equal(_png16_read(res / (RAW + ".png")), want)
    assert not np.array_equal(want, _binding(lay, t_emap, t_tiles, None)[0])
    lines = _weights_lines(r.stdout)
    _check_lines(lines, sm, lay)
    if kind == "tent":  # every sample has a positive weight
        assert all(re.search(r": (\d+) of \1 samples", ln) for ln in lines), lines
    else:  # tile 0 lost its rectangle's samples
        assert not re.search(r": (\d+) of \1 samples", lines[0]), lines[0]


def test_the_tent_of_the_binding_is_the_formula(folder):
    _, lay, _, _, _, _ = folder
    fz = panofuse.Fuser(0)
    fz.set_tiles(lay)
    got = fz.tent_weights().cpu().numpy()
    fz.close()
    assert np.array_equal(got, WR.tent(O.make_tiles(lay)[0]))


def test_a_weight_file_of_another_size_is_refused(folder):
    run = folder[0]
    r, res = run("badsize", "--tile-weights", "files:" + SUFFIX, tiles_dir="badtiles")
    assert not (res / (RAW + ".png")).exists(), r.stdout
    lines = [ln for ln in r.stdout.splitlines() if "weight map" in ln]
    assert len(lines) == 1 and lines[0].endswith(f"{SUFFIX} is 247x256, its tile 256x247"), r.stdout
    assert PL.tile_names(folder[1])[3] in lines[0]
    r, res = run("nofile", "--tile-weights", "files:.missing.pfm")
    assert not (res / (RAW + ".png")).exists() and ".missing.pfm" in r.stdout, r.stdout


def test_refused_next_to_another_mode(folder):
    """Before any GPU call: exit status 2, one line, no result (every pair:
    tests/test_weights_sanitized.py); and the facade's own refusal under the environment."""
    run = folder[0]
    r, res = run("clash", "--tile-weights", "tent", "--tile-valid", "0:inf")
    assert (r.returncode, r.stdout) == (
        2, "--tile-weights registers and fuses with per-pixel weights: not with --tile-valid\n")
    assert not (res / (RAW + ".png")).exists()
    r, res = run("clash_env", "--tile-valid", "0:inf", env_extra={"PF_TILE_WEIGHTS": "tent"})
    assert "tile weights (PF_TILE_WEIGHTS / SetTileWeights) have no form for the tile validity " \
           "rule" in r.stdout, r.stdout
    assert not (res / (RAW + ".png")).exists()
    r, res = run("bad_env", env_extra={"PF_TILE_WEIGHTS": "tents"})
    assert "PF_TILE_WEIGHTS: bad tile weights \"tents\"" in r.stdout
    assert not (res / (RAW + ".png")).exists()


def test_without_the_flag_nothing_changes(folder):
    run, lay, t_emap, t_tiles, _, _ = folder
    r, res = run("plain")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "[weights]" not in r.stdout
    assert np.array_equal(_png16_read(res / (RAW + ".png")), _binding(lay, t_emap, t_tiles, None)[0])
    # the files a weighted run writes are the files a plain run writes
    r2, res2 = run("tent_files", "--tile-weights", "tent")
    assert r2.returncode == 0, r2.stdout + r2.stderr
    assert sorted(os.listdir(res)) == sorted(os.listdir(res2))

    def stable(text, res_dir):  # without this run's folder, the numbers and the [weights] lines
        text = "\n".join(ln for ln in text.splitlines() if not ln.startswith("[weights]"))
        return re.sub(r"[-+]?\d[\d.e+-]*", "N", text.replace(str(res_dir), "RES"))
    assert stable(r.stdout, res) == stable(r2.stdout, res2)


@pytest.mark.parametrize("kind", ["tent", "files"])
def test_set_tile_weights_from_cpp(folder, kind, tmp_path):
    """SetTileWeights + MergeDepthMaps from compiled C++ (tests/cpp/weights_link.cpp)."""
    _, lay, t_emap, t_tiles, field, files = folder
    out = tmp_path / "linked.png"
    mode, suffix = ("1", "-") if kind == "tent" else ("2", SUFFIX)
    env = {k: v for k, v in os.environ.items() if k not in ENV_DROP}
    r = subprocess.run([LINK, mode, suffix, "512", files["base"], str(out)] + files["tiles"],
                       capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    for tag in ("BADMODE refused", "NOSUFFIX refused", "MERGED 1", "WITHRULE refused"):
        assert tag in r.stdout.splitlines(), r.stdout
    assert r.stdout.count("[SetTileWeights]") == 2
    want, sm = _binding(lay, t_emap, t_tiles, "tent" if kind == "tent" else field)
    assert np.array_equal(_png16_read(out), want)
    _check_lines(_weights_lines(r.stdout), sm, lay)
    assert not (tmp_path / "linked.png.rule.png").exists()
