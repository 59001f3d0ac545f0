"""GPU end-to-end of the disparity tiles' per-pixel weights on the command line and through the
facade.

Mode 0 on a C1-sized folder (512x256 output, 128x64 baseline, the default table's 15 tiles at
256x247 as 16-bit PNGs of per-tile normalised inverse depth whose top 110 rows are disparity 0, the
"sky" a network writes; the pattern of tests/test_gpu_weights_cli.py): with --tile-model disparity
--disparity-weights tent, range:0:inf and files:.w.pfm, by the flag and by PF_DISPARITY_WEIGHTS,
the result PNG equals the binding's merge_disparity_weighted byte for byte and the "[weights]"
lines carry register_disparity_weighted's summary; without the flag the run writes what it always
wrote.  tests/cpp/disp_weights_link.cpp calls SetDisparityWeights + MergeDisparityMaps from
compiled C++ on the same folder.  Every clashing pair of flags runs without a GPU in
tests/test_disp_weights_sanitized.py."""
import os
import re
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import panofuse  # noqa: E402
import pf_layouts as PL  # noqa: E402
from test_disp_weights_sanitized import ENV_DROP  # noqa: E402
from test_gpu_disp_cli import _png16_read, _png16_write, _q16, _scene  # noqa: E402
from test_gpu_weights_cli import _field, _pfm_write  # noqa: E402

PKG = os.path.dirname(os.path.dirname(panofuse.LIB_PATH))
MAIN = os.path.join(PKG, "bin", "panofuse_main")
LINK = os.path.join(PKG, "bin", "pf_disp_weights_link")
ZR = PL.ZENITH_RANGE
DEV = "cuda:0"
RAW = "scene01_rgb"
TW, TH = 256, 247
SUFFIX = ".w.pfm"
SKY_ROWS = 110
SPECS = {"tent": "tent", "range": "range:0:inf", "files": "files:" + SUFFIX}


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected on a host without a GPU")
    root = tmp_path_factory.mktemp("disp_weights_cli")
    d = {k: root / k for k in ("rgb", "gt", "base", "tiles")}
    for p in d.values():
        p.mkdir()
    lay = PL.leres_layout(TW, TH)
    tiles, gt, base, disp = _scene(lay, 20261021 + 91, 512, 128)
    (d["rgb"] / (RAW + ".jpg")).write_bytes(b"\xff\xd8")  # only the name is used
    tq = _q16(disp).reshape(lay.ntiles, TH, TW).copy()
    tq[:, :SKY_ROWS, :] = 0
    bq = _q16(base).copy()
    _png16_write(d["gt"] / (RAW.replace("_rgb", "_depth") + ".png"), _q16(gt))
    _png16_write(d["base"] / (RAW + ".depth.png"), bq)
    names = PL.tile_names(lay)
    field = _field(lay)
    for t in range(lay.ntiles):
        _png16_write(d["tiles"] / f"{RAW}.{names[t]}.png", tq[t])
        _pfm_write(d["tiles"] / f"{RAW}.{names[t]}.png{SUFFIX}", field[t])

    def run(tag, *opts, env_extra=None):
        res = root / tag / "result_hohonet"
        res.mkdir(parents=True)
        cmd = [MAIN, "0", str(d["rgb"]), str(d["gt"]), str(d["base"]), str(res), "--tiles",
               str(d["tiles"]), "--ext", "png", "--width", "512", "--tile-model",
               "disparity"] + list(opts)
        env = {k: v for k, v in os.environ.items() if k not in ENV_DROP}
        env.update(env_extra or {})
        return subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=env), res

    t_emap = torch.from_numpy(bq.astype(np.float32) / np.float32(65535.0))[None].to(DEV)
    t_tiles = torch.from_numpy((tq.astype(np.float32) / np.float32(65535.0)).reshape(1, -1)).to(DEV)
    files = {"base": str(d["base"] / (RAW + ".depth.png")),
             "tiles": [str(d["tiles"] / f"{RAW}.{names[t]}.png") for t in range(lay.ntiles)]}
    return run, lay, t_emap.contiguous(), t_tiles.contiguous(), field, files


_CACHE = {}


def _binding(lay, t_emap, t_tiles, kind, field=None, planar=False):
    """(u16 result, summary [ntiles][6]) of merge_disparity_weighted /
    register_disparity_weighted; kind None: the plain merge_disparity.  Computed once."""
    key = (kind, planar)
    if key in _CACHE:
        return _CACHE[key]
    fz = panofuse.Fuser(0)
    fz.set_tiles(lay)
    if planar:
        fz.set_tile_depth("planar")
    out = torch.zeros((1, 256, 512), dtype=torch.int16, device=DEV)
    sm = torch.zeros((1, lay.ntiles, 6), dtype=torch.float64, device=DEV)
    if kind is None:
        fz.merge_disparity(t_emap, t_tiles, out, ZR)
    else:
        w = {"tent": lambda: fz.tent_weights(),
             "range": lambda: fz.range_weights(t_tiles, 0.0, float("inf")),
             "files": lambda: torch.from_numpy(np.ascontiguousarray(field).reshape(-1)).to(DEV)
             }[kind]()
        fz.merge_disparity_weighted(t_emap, t_tiles, w, out, ZR)
        fz.register_disparity_weighted(t_emap, t_tiles, w, ZR, apply=False, summary=sm)
    fz.synchronize()
    fz.close()
    _CACHE[key] = (out.cpu().numpy().view(np.uint16)[0], sm.cpu().numpy()[0])
    return _CACHE[key]


def _weights_lines(stdout):
    return [ln for ln in stdout.splitlines() if ln.startswith("[weights]")]


def _check_lines(lines, sm, lay):
    assert len(lines) == lay.ntiles
    for p, ln in enumerate(lines):
        m = re.fullmatch(r"\[weights\] tile (\d+): (\d+) of (\d+) samples used, sum w (\S+)", ln)
        assert m, ln
        assert (int(m.group(1)), int(m.group(2))) == (p, int(sm[p, 4])), ln
        assert int(m.group(3)) >= int(m.group(2)) >= 3
        assert m.group(4) == "%.6g" % sm[p, 5], ln


@pytest.mark.parametrize("how", ["flag", "env"])
@pytest.mark.parametrize("kind", ["tent", "range", "files"])
def test_disparity_weights(folder, kind, how):
    run, lay, t_emap, t_tiles, field, _ = folder
    if how == "flag":
        r, res = run(f"{kind}_flag", "--disparity-weights", SPECS[kind])
    else:
        r, res = run(f"{kind}_env", env_extra={"PF_DISPARITY_WEIGHTS": SPECS[kind]})
    assert r.returncode == 0, r.stdout + r.stderr
    want, sm = _binding(lay, t_emap, t_tiles, kind, field)
    assert np.array_equal(_png16_read(res / (RAW + ".png")), want)
    assert not np.array_equal(want, _binding(lay, t_emap, t_tiles, None)[0])
    lines = _weights_lines(r.stdout)
    _check_lines(lines, sm, lay)
    if kind == "tent":  # every sample has a positive weight
        assert all(re.search(r": (\d+) of \1 samples", ln) for ln in lines), lines
    if kind == "range":  # the sky's samples are off, and every weight is 1
        assert not all(re.search(r": (\d+) of \1 samples", ln) for ln in lines), lines
        assert np.array_equal(sm[:, 4], sm[:, 5])


def test_planar_tiles_are_accepted(folder):
    run, lay, t_emap, t_tiles, _, _ = folder
    r, res = run("planar", "--disparity-weights", "range:0:inf", "--tile-depth", "planar")
    assert r.returncode == 0, r.stdout + r.stderr
    want, sm = _binding(lay, t_emap, t_tiles, "range", planar=True)
    assert np.array_equal(_png16_read(res / (RAW + ".png")), want)
    assert not np.array_equal(want, _binding(lay, t_emap, t_tiles, "range")[0])
    _check_lines(_weights_lines(r.stdout), sm, lay)
    assert "[tile-depth] planar" in r.stdout


def test_refusals_of_the_facade(folder):
    """The flag pairs exit 2 before any GPU call (tests/test_disp_weights_sanitized.py); here the
    facade's own refusals under the environment, before any file is read, and the refusal of
    --tile-weights with disparity tiles, which stays what it was."""
    run = folder[0]
    r, res = run("clash_env", "--tile-valid", "0:inf",
                 env_extra={"PF_DISPARITY_WEIGHTS": "range:0:inf"})
    assert "disparity weights (PF_DISPARITY_WEIGHTS / SetDisparityWeights) fit and fuse " \
           "disparity tiles with per-pixel weights: not with PF_TILE_VALID / SetTileValidity" \
           in r.stdout, r.stdout
    assert not (res / (RAW + ".png")).exists()
    r, res = run("bad_env", env_extra={"PF_DISPARITY_WEIGHTS": "range:1:0"})
    assert "PF_DISPARITY_WEIGHTS: bad disparity weights \"range:1:0\"" in r.stdout
    assert not (res / (RAW + ".png")).exists()
    r, res = run("tile_weights_env", env_extra={"PF_TILE_WEIGHTS": "tent"})
    assert "tile weights (PF_TILE_WEIGHTS / SetTileWeights) have no form for disparity tiles" \
           in r.stdout, r.stdout
    assert not (res / (RAW + ".png")).exists()


def test_without_the_flag_nothing_changes(folder):
    run, lay, t_emap, t_tiles, _, _ = folder
    r, res = run("plain")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "[weights]" not in r.stdout
    assert np.array_equal(_png16_read(res / (RAW + ".png")),
                          _binding(lay, t_emap, t_tiles, None)[0])
    # the files a weighted run writes are the files a plain run writes
    r2, res2 = run("tent_files", "--disparity-weights", "tent")
    assert r2.returncode == 0, r2.stdout + r2.stderr
    assert sorted(os.listdir(res)) == sorted(os.listdir(res2))

    def stable(text, res_dir):  # without this run's folder, the numbers and the [weights] lines
        text = "\n".join(ln for ln in text.splitlines() if not ln.startswith("[weights]"))
        return re.sub(r"[-+]?\d[\d.e+-]*", "N", text.replace(str(res_dir), "RES"))
    assert stable(r.stdout, res) == stable(r2.stdout, res2)


@pytest.mark.parametrize("kind", ["tent", "range", "files"])
def test_set_disparity_weights_from_cpp(folder, kind, tmp_path):
    """SetDisparityWeights + MergeDisparityMaps from compiled C++ (tests/cpp/
    disp_weights_link.cpp)."""
    _, lay, t_emap, t_tiles, field, files = folder
    out = tmp_path / "linked.png"
    mode, arg = {"tent": ("1", "-"), "range": ("3", "0:inf"), "files": ("2", SUFFIX)}[kind]
    env = {k: v for k, v in os.environ.items() if k not in ENV_DROP}
    r = subprocess.run([LINK, mode, arg, "512", files["base"], str(out)] + files["tiles"],
                       capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    for tag in ("BADMODE refused", "BADRANGE refused", "MERGED 1", "DEPTHTILES refused",
                "WITHRULE refused"):
        assert tag in r.stdout.splitlines(), r.stdout
    assert r.stdout.count("[SetDisparityWeights]") == 2
    want, sm = _binding(lay, t_emap, t_tiles, kind, field)
    assert np.array_equal(_png16_read(out), want)
    _check_lines(_weights_lines(r.stdout), sm, lay)
    assert not (tmp_path / "linked.png.rule.png").exists()
    assert not (tmp_path / "linked.png.depth.png").exists()
