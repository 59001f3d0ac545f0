"""GPU end-to-end of the edge metrics on the command line: `panofuse_main lap` (the reference's
ErrorLaplacian on two files, Depth.cpp:2636-2953) and the opt-in `--edge-metrics` flag of mode 0
(<raw>.edges.txt beside <raw>.aligned.txt)."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import edge_ref as E  # noqa: E402
import panofuse  # noqa: E402
import pf_layouts as PL  # noqa: E402
import pf_synth  # noqa: E402
import pyoracle as O  # noqa: E402

BIN = os.path.join(os.path.dirname(os.path.dirname(panofuse.LIB_PATH)), "bin", "panofuse_main")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "edge_metrics_ref.npz")
MYPI = 3.14159265359


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected on a host without a GPU")


def _six_digits(v):
    """A double as std::cout prints it at the default precision (%g)."""
    return float("%g" % v)


def test_lap_command_on_a_golden_pair(tmp_path):
    """Pair 2 (gt 100 x 50 against a given map of 64 x 33): the printed line carries the
    reference's doubles to the six digits it prints, and the counts follow."""
    _need_gpu()
    z = np.load(GOLDEN)
    gfn, vfn = str(tmp_path / "gt.png"), str(tmp_path / "given.png")
    E.write_png16(gfn, z["gt2"])
    E.write_png16(vfn, z["given2"])
    r = subprocess.run([BIN, "lap", gfn, vfn], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"\[ErrorLap\] Lap_mse:(\S+) Lap_mae:(\S+) SobelX:(\S+) SobelY:(\S+) Lap5x5:(\S+)",
                  r.stdout)
    assert m, r.stdout
    for i in range(5):
        assert float(m.group(i + 1)) == _six_digits(float(z["ref2"][i])), (i, m.group(i + 1))
    c = re.search(r"\[ErrorLap\] n_lap:(\d+) n_sobel:(\d+) n_lap5:(\d+)", r.stdout)
    assert c, r.stdout
    assert [int(c.group(i + 1)) for i in range(3)] == z["counts2"].tolist()
    # a file that does not load: the reference's message and a failure exit code
    r = subprocess.run([BIN, "lap", gfn, str(tmp_path / "missing.png")], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 1 and "cannot load emap_baseline? " in r.stdout


def _cround(x):
    return int(math.copysign(math.floor(abs(x) + 0.5), x))


def _q16(a):
    return (np.clip(a, 0, 1) * 65535.0 + 0.5).astype(np.uint16)


def test_mode0_edge_metrics_flag(tmp_path):
    """One scene through mode 0 without and with --edge-metrics: no .edges.txt without the flag;
    with it, the file's values are the restatement's for the written result and for the baseline
    against the gt, up to the six decimals of "%f"."""
    _need_gpu()
    d = {k: tmp_path / k for k in ("rgb", "gt", "base", "plain_hohonet", "edges_hohonet", "tiles")}
    for p in d.values():
        p.mkdir()
    lay = PL.leres_layout(512, 494)
    tiles_o, total = O.make_tiles(lay)
    raw = "scene01_rgb"
    (d["rgb"] / (raw + ".jpg")).write_bytes(b"\xff\xd8")  # only the name is used
    seeds = pf_synth.seeds_for(1, 20261019 + 5)
    gt = _q16(pf_synth.scene_depth(seeds, 2048, 1024)[0].numpy())
    gt[60:64, 500:1500] = 0  # black pixels inside the compared region
    base = _q16(pf_synth.baseline_emap(seeds, 512, 256)[0].numpy())
    E.write_png16(d["gt"] / (raw.replace("_rgb", "_depth") + ".png"), gt)
    E.write_png16(d["base"] / (raw + ".depth.png"), base)  # hohonet naming (Main.cpp:512-516)
    gt_f = E.u16_to_float(gt)
    tq = _q16(O.warp_depth(gt_f, tiles_o, total, O.responses(pf_synth.responses(seeds, lay.ntiles))))
    n = 512 * 494
    for t in range(lay.ntiles):
        f = [_cround(float(v) / MYPI * 180.0) for v in lay.fovs[t]]
        E.write_png16(d["tiles"] / f"{raw}.{f[0]}_{f[1]}_{f[2]}_{f[3]}.png",
                      tq[t * n:(t + 1) * n].reshape(494, 512))

    def run(result, extra):
        r = subprocess.run([BIN, "0", str(d["rgb"]), str(d["gt"]), str(d["base"]), str(result),
                            "--tiles", str(d["tiles"])] + extra, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert (result / (raw + ".png")).exists() and (result / (raw + ".aligned.txt")).exists()
        return r.stdout

    plain = run(d["plain_hohonet"], [])
    assert not (d["plain_hohonet"] / (raw + ".edges.txt")).exists()
    assert "[ErrorLap]" not in plain
    # the flag takes no value: options after it are still read
    run(d["edges_hohonet"], ["--edge-metrics", "--metrics-order", "tree"])
    txt = (d["edges_hohonet"] / (raw + ".edges.txt")).read_text()
    vals = dict(line.split(": ") for line in txt.strip().splitlines())
    result = E.read_png16(d["edges_hohonet"] / (raw + ".png"))
    assert np.array_equal(result, E.read_png16(d["plain_hohonet"] / (raw + ".png")))
    for tag, given in (("result", E.u16_to_float(result)), ("given", E.u16_to_float(base))):
        ref = E.edge_metrics(gt_f, given)
        for k in E.KEYS:
            assert abs(float(vals[f"{k}_{tag}"]) - ref[k]) <= 5.01e-7, (tag, k, vals[f"{k}_{tag}"], ref[k])
        for k in E.COUNTS:
            assert int(vals[f"{k}_{tag}"]) == ref[k] > 0, (tag, k)
    assert len(vals) == 16
