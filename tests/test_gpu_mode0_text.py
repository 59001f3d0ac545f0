"""What mode 0 prints and which files it writes, line by line -- GPU, two runs of the tiny folder
of tests/test_gpu_global_cli.py / test_gpu_stitch_cli.py (512x256 output, 128x64 baseline, LeReS'
15 windows with 256x247 tiles, one panorama): plain, and with every diagnostic switched on.

stdout is compared with the text below after every number has become `#` and the temporary
directory `<tmp>`, so the test pins the order and the wording of the lines (the reference-style
diagnostics, [SolveDepthToDepth2], [ErrorLap], [layout], time_Reg:, the averages); the values are
held bit for bit by the other CLI tests."""
import os
import re
import subprocess

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import pf_layouts as PL  # noqa: E402
import pf_synth  # noqa: E402
import pyoracle as O  # noqa: E402
from test_gpu_global_cli import MAIN, MYPI, _cround, _png16_write, _q16  # noqa: E402

RAW = "scene01_rgb"
SWITCHES = ("PF_FUSION", "PF_SAVE_STITCH", "PF_CHECK_LAPLACIAN", "PF_GLOBAL_ALIGN", "PF_LAYOUT",
            "PF_EDGE_METRICS", "PF_TILE_MODEL", "PF_METRICS_ORDER")
NUMBER = re.compile(r"[-+]?(?:\d+\.?\d*(?:e[-+]?\d+)?|nan|inf)")

HEAD = """\
[CreateDepthPanormas] #RGB_filenames:#
#/# baseline:<tmp>/base/scene#_rgb.depth.png
gt:<tmp>/gt/scene#_depth.png
output_filename:<tmp>/{run}/result_hohonet/scene#_rgb.png
"""
DONE = """\
...All done! @#
RMSE #-># (#) MAE #-># (#) MRE #-># (#) RMSElog #-># (#) deltas:#->#(#) , #->#(#) , #->#(#
[layout] level # (#x#): # taps outside their tile (clamped)
"""
TAIL = """\
time_Reg:# time_Laplacian:#
RMSE_given:# RMSE_result:# MAE_given:# MAE_result_avg:# delta#_given:# delta#_result:#
"""
PLAIN = HEAD + DONE + TAIL
FULL = HEAD + """\

[SolveDepthAll] check Laplacian err:#
[SolveDepthToDepth#] abcd:(# # # #) cost:#->#
""" + DONE + """\
[ErrorLap] Lap_mse:# Lap_mae:# SobelX:# SobelY:# Lap#x#:#
[ErrorLap] Lap_mse:# Lap_mae:# SobelX:# SobelY:# Lap#x#:#
""" + TAIL
PLAIN_FILES = [RAW + ".aligned.txt", RAW + ".png", RAW + ".png.giv.png", RAW + ".png.res.png"]
FULL_FILES = sorted(PLAIN_FILES + [RAW + ".edges.txt", RAW + ".png.pmap.png"])


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected on a host without a GPU")
    root = tmp_path_factory.mktemp("mode0_text")
    d = {k: root / k for k in ("rgb", "gt", "base", "tiles")}
    for p in d.values():
        p.mkdir()
    tw, th = 256, 247
    lay = PL.leres_layout(tw, th)
    tiles, total = O.make_tiles(lay)
    seeds = pf_synth.seeds_for(1, 20261020 + 5)
    gt = pf_synth.scene_depth(seeds, 512, 256)[0].numpy()
    base = pf_synth.baseline_emap(seeds, 128, 64)[0].numpy()
    tq = _q16(O.warp_depth(gt, tiles, total, O.responses(pf_synth.responses(seeds, lay.ntiles))))
    (d["rgb"] / (RAW + ".jpg")).write_bytes(b"\xff\xd8")  # only the name is used
    _png16_write(d["gt"] / (RAW.replace("_rgb", "_depth") + ".png"), _q16(gt))
    _png16_write(d["base"] / (RAW + ".depth.png"), _q16(base))  # hohonet naming
    for t in range(lay.ntiles):
        f = [_cround(float(v) / MYPI * 180.0) for v in lay.fovs[t]]
        _png16_write(d["tiles"] / f"{RAW}.{f[0]}_{f[1]}_{f[2]}_{f[3]}.png",
                     tq[t * tw * th:(t + 1) * tw * th].reshape(th, tw))

    def run(name, *flags):
        res = root / name / "result_hohonet"
        res.mkdir(parents=True)
        cmd = [MAIN, "0", str(d["rgb"]), str(d["gt"]), str(d["base"]), str(res), "--tiles",
               str(d["tiles"]), "--ext", "png", "--width", "512", *flags]
        env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0, r.stdout + r.stderr
        text = NUMBER.sub("#", r.stdout.replace(str(root), "<tmp>"))
        print(f"---- {name} ----\n{text}")
        return text.splitlines(), sorted(p.name for p in res.iterdir())
    return run


@pytest.mark.parametrize("name,flags,text,files", [
    ("plain", (), PLAIN, PLAIN_FILES),
    ("full", ("--global-align", "--save-stitch", "--check-laplacian", "--edge-metrics"), FULL,
     FULL_FILES)])
def test_mode0_lines_and_files(folder, name, flags, text, files):
    lines, written = folder(name, *flags)
    assert lines == text.format(run=name).splitlines()
    assert written == files
