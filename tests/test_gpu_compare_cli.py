"""GPU end-to-end of `panofuse_main cmp` (the reference's ErrorCompare on two files,
Depth.cpp:2460-2634) on two cases of tests/golden/compare_ref.npz: one in depth mode, one with a
mono360 PFM baseline in disparity mode.  The printed CMP line carries the reference's seven floats
under the bars of tests/test_gpu_metrics.py (bit-exact at %.9g; mselog within 1e-5 relative), and
the saved PNG is the reference's file byte for byte.  A file that does not load ends the command
with exit code 1."""
import math
import os
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import compare_ref as R  # noqa: E402
import panofuse  # noqa: E402
import pf_layouts as PL  # noqa: E402

BIN = os.path.join(os.path.dirname(os.path.dirname(panofuse.LIB_PATH)), "bin", "panofuse_main")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "compare_ref.npz")
LOG_RTOL = 1e-5


def _case(cases, **want):
    hit = [c for c in cases if all(c[k] == v for k, v in want.items())]
    assert hit, want
    return hit[0]


def _run_cmp(tmp_path, c):
    gfn = str(tmp_path / ("gt" + R.extension(c["gt_kind"])))
    vfn = str(tmp_path / ("given" + R.extension(c["given_kind"])))
    sfn = str(tmp_path / "shifted.png")
    R.write_file(gfn, c["gt_raw"], c["gt_kind"])
    R.write_file(vfn, c["given_raw"], c["given_kind"])
    args = [BIN, "cmp", gfn, vfn, "--align", str(c["align_way"]), "--save", sfn]
    if c["disp"]:
        args.append("--disp")
    if not c["cap"]:
        args.append("--no-cap")
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout, sfn


def _check_cmp_line(out, c):
    line = [ln for ln in out.splitlines() if ln.startswith("CMP ")]
    assert len(line) == 1, out
    got = [float(np.float32(t)) for t in line[0].split()[1:]]
    assert len(got) == 7
    for m, a, b in zip(R.METRICS, got, c["ref"].tolist()):
        same = (math.isnan(a) and math.isnan(b)) or a == b
        if m == "mselog":
            assert same or abs(a - b) <= LOG_RTOL * abs(b), (m, a, b)
        else:
            assert same, (m, a, b)


def test_cmp_depth_mode(tmp_path):
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected on a host without a GPU")
    c = _case(R.golden_cases(np.load(GOLDEN)), pair=1, disp=False, align_way=1, cap=True)
    out, sfn = _run_cmp(tmp_path, c)
    _check_cmp_line(out, c)
    assert "FIT " not in out
    assert f"[ErrorCompare] 1 saved shifted emap:{sfn}" in out
    assert open(sfn, "rb").read() == c["png"]


def test_cmp_disparity_pfm_and_missing_file(tmp_path):
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected on a host without a GPU")
    c = _case(R.golden_cases(np.load(GOLDEN)), pair=7, disp=True, align_way=0, cap=True)
    assert c["given_kind"] == "pfm" and c["gt_raw"].ndim == 3
    out, sfn = _run_cmp(tmp_path, c)
    _check_cmp_line(out, c)
    assert open(sfn, "rb").read() == c["png"]
    fit = [ln for ln in out.splitlines() if ln.startswith("FIT ")]
    assert len(fit) == 1, out
    s, o, vmin, vmax, n = fit[0].split()[1:]
    ref = R.compare(R.load_map(c["gt_raw"], c["gt_kind"]),
                    R.load_map(c["given_raw"], c["given_kind"], True), PL.ZENITH_RANGE, True, 0, True)
    assert [float(np.float32(t)) for t in (s, o, vmin, vmax)] == \
        [ref["fit_s"], ref["fit_o"], ref["vmin"], ref["vmax"]]
    assert int(n) == ref["n_nonblack"]
    # a file that does not load: the reference's message and exit code 1, nothing written
    gfn = str(tmp_path / "gt.png")
    for args, msg in (([gfn, str(tmp_path / "missing.pfm")], "cannot load emap_baseline? "),
                      ([str(tmp_path / "missing.png"), gfn], "cannot load emap_gt? ")):
        r = subprocess.run([BIN, "cmp"] + args + ["--disp", "--save", str(tmp_path / "no.png")],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and msg in r.stdout, r.stdout + r.stderr
        assert "CMP " not in r.stdout and not (tmp_path / "no.png").exists()
