"""CPU checks of the edge-fidelity metrics (ErrorLaplacian, Depth.cpp:2636-2953).

* The numpy fp64 restatement (tests/edge_ref.py) against tests/golden/edge_metrics_ref.npz: five
  small 16-bit PNG pairs with the five doubles that the reference's own compiled ErrorLaplacian
  returned for them (tools/make_edge_golden.py; printed at %.17g).  Bar: each mean within
  2 * N * 2^-53 relative (N = w * h of the given map) -- the reference's column-major fp64 sum
  and the restatement's exact sum both lie within (N - 1) * 2^-53 of the exact value, and the
  per-sample terms are the same doubles.  Recorded: worst 3.7e-14 against bounds of 4.5e-13 and up.
* The libraries export the new entry points: pf_error_laplacian (C-ABI) and
  DepthNamespace::ErrorLaplacian with the reference's signature (Depth.h:321-323), so a caller
  compiled against the reference's header links against the facade."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import edge_ref as E
import panofuse

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "edge_metrics_ref.npz")
NPAIRS = 5


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("k", range(NPAIRS))
def test_restatement_matches_reference(golden, k):
    g16, v16 = golden[f"gt{k}"], golden[f"given{k}"]
    ref, counts = golden[f"ref{k}"], golden[f"counts{k}"]
    h, w = v16.shape
    got = E.edge_metrics(E.u16_to_float(g16), E.u16_to_float(v16))
    assert [got[c] for c in E.COUNTS] == counts.tolist()
    assert min(counts) > 0
    for i, key in enumerate(E.KEYS):
        print(key, got[key], float(ref[i]), abs(got[key] - ref[i]) / abs(ref[i]), E.mean_bound(w, h))
        assert E.close(got[key], float(ref[i]), w, h), (key, got[key], float(ref[i]))


def test_golden_covers_the_ratios(golden):
    shapes = [(golden[f"gt{k}"].shape, golden[f"given{k}"].shape) for k in range(NPAIRS)]
    assert shapes == [((32, 64), (32, 64)), ((64, 128), (32, 64)), ((50, 100), (33, 64)),
                      ((33, 64), (50, 100)), ((37, 75), (37, 75))]
    for k in range(NPAIRS):
        g = golden[f"gt{k}"]
        band = max(2, g.shape[0] // 10)
        assert not g[:band].any()                      # the zero band
        assert 0.02 < (g[band:] == 0).mean() < 0.05    # ~3 % black pixels below it
    assert os.path.getsize(GOLDEN) < 100 * 1024


def test_restatement_sobel_list_is_the_references():
    """A gt whose only invalid pixel sits at val[1][0] (above the centre): the reference's Sobel
    list never tests it, the Laplacian's does."""
    gt = np.full((7, 7), 0.5, np.float32)
    gt[2, 3] = 0.0
    given = np.full((7, 7), 0.4, np.float32)
    loose = E.edge_metrics(gt, given)
    strict = E.edge_metrics(gt, given, strict_sobel=True)
    # 25 3x3 samples; the zero is a tap of the 9 samples around it: all 9 under the strict
    # test, 7 under the reference's (not where it is val[1][0] or val[2][0])
    assert strict["n_sobel"] == 25 - 9 and loose["n_sobel"] == 25 - 7
    assert loose["n_lap"] == 25 - 5


def test_c_abi_exports_pf_error_laplacian():
    lib = C.CDLL(panofuse.LIB_PATH)
    assert hasattr(lib, "pf_error_laplacian")
    assert "pf_error_laplacian" in panofuse.EXPORTS


def test_facade_exports_the_reference_signature():
    lib = os.path.join(os.path.dirname(panofuse.LIB_PATH), "libpanofuse_depth.so")
    out = subprocess.run(["nm", "-DC", lib], capture_output=True, text=True, check=True).stdout
    s = "std::__cxx11::basic_string<char, std::char_traits<char>, std::allocator<char> >"
    want = (f"DepthNamespace::ErrorLaplacian({s}&, {s}&, double&, double&, double&, double&, "
            f"double&, {s}*, {s}*, {s}*)")
    assert any(line.endswith(" T " + want) for line in out.splitlines()), want
