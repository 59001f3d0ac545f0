"""The HIP library against the compiled reference on the registration / fusion / smoothing path.

Reads tests/golden/fusion_ref.npz only (tools/make_fusion_golden.py: the reference's own
SolveDepthToDepth with real Ceres 1.13, Depth2DepthTransform, SolveDepthAll,
SolveDepthBySmoothing and ErrorData; cases and bars in tests/fusion_ref.py).  The oracle is used
for one thing, the registration samples from which a tile's condition number is computed; no
expected value comes from it.

Bars, the same as the CPU oracle's in tests/test_fusion_ref.py: coefficients the same bits on
well-conditioned tiles and within 1e-5 relative on ill-conditioned ones and on the joint sets;
transformed tiles every bit; panoramas every u16; six ErrorData floats every bit and mselog
within test_gpu_metrics.py's 1e-5 (its log10f is the device's).

The sizes are small, which is the point: their levels take the Jacobi engines the 512- and
2048-wide parity tests never reach.  fusion_ref.ENGINES lists, per case and level, the engine
(per-sweep kernel "sweeps", "streamed", "resident"), the form ("packed" / "general") and whether
the target patches are partial; tests/test_fusion_ref.py derives the table from the host's rules.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import fusion_ref as F  # noqa: E402
import panofuse  # noqa: E402
from test_fusion_ref import GOLDEN, MERGE  # noqa: E402

DEV = "cuda:0"
LOG_RTOL = 1e-5  # tests/test_gpu_metrics.py: mselog in sequential order
HALF = [c for c in MERGE if F.CASES[c][4][1] == F.CASES[c][4][0] // 2 and c not in F.SPLIT]


@pytest.fixture(scope="module")
def fuser():
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected on a host without a GPU")
    return panofuse.Fuser(0)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


_results = {}


def _register_and_fuse(fuser, golden, case):
    """pf_register (LM, apply=True) then pf_fuse of the transformed tiles, once per case:
    (coeffs [n][4], transformed tiles, u16 [H][W], kappas)."""
    if case not in _results:
        lay, tiles, data, emap, (W, H), zr = F.case_inputs(golden, case)
        fuser.set_tiles(lay)
        t_emap, t_tiles = _dev(emap)[None], _dev(data)[None].contiguous()
        coeffs = torch.zeros((1, lay.ntiles, 4), dtype=torch.float32, device=DEV)
        out = torch.zeros((1, H, W), dtype=torch.int16, device=DEV)
        if case in F.SPLIT:  # fusion_ref.SPLIT: the transform from the recorded coefficients
            fuser.register(t_emap, t_tiles, zr, degree=3, apply=False, coeffs=coeffs)
            fuser.fuse(t_emap, t_tiles, out, zr, coeffs=_dev(golden[case + "_abcd"])[None])
        else:
            fuser.register(t_emap, t_tiles, zr, degree=3, apply=True, coeffs=coeffs)
            fuser.fuse(t_emap, t_tiles, out, zr)
        fuser.synchronize()
        _results[case] = (coeffs.cpu().numpy()[0], t_tiles.cpu().numpy()[0], _u16(out)[0],
                          F.tile_kappas(tiles, data, emap, zr))
    return _results[case]


@pytest.mark.parametrize("case", MERGE)
def test_register_then_fuse(fuser, golden, case):
    """pf_register (the LM solver, apply=True) and pf_fuse at every merge case, the sizes whose
    height is not half the width included (500x248, 384x160).  Engines per level
    (fusion_ref.ENGINES): 256x128 sweeps / streamed / resident; 200x100 sweeps / sweeps /
    streamed with partial patches at every level; 500x248 sweeps (odd width 125) / streamed /
    streamed, partial; 384x160 sweeps (partial) / streamed / streamed; LERES 512x256 streamed /
    resident / resident; the wide band the general form at every level (sweeps / streamed /
    streamed).  On the narrow-range LERES case the tiles stay untransformed and pf_fuse applies
    the recorded coefficients on the fly (fusion_ref.SPLIT)."""
    abcd, tt, out, kap = _register_and_fuse(fuser, golden, case)
    ref = golden[case + "_abcd"]
    print(f"{case}: abcd up to {int(F.ulp_diff(abcd, ref).max())} ulp, rel "
          f"{float(F.rel_diff(abcd, ref).max()):.3g}")
    assert F.abcd_mismatch(abcd, ref, kap, case in F.SPLIT) == []
    n, (tw, th) = len(kap), F.CASES[case][2]
    if case not in F.SPLIT:
        assert F.plane_mismatch(golden, case + "_tiles", F.bits(tt).reshape(n, th, tw)) == 0
    assert F.plane_mismatch(golden, case + "_out", out) == 0


@pytest.mark.parametrize("case", HALF)
def test_merge_batch1(fuser, golden, case):
    """pf_merge, one panorama, on the cases whose height is half the width (the 256x128 ones,
    200x100 and LERES 512x256; engines as in test_register_then_fuse)."""
    lay, tiles, data, emap, (W, H), zr = F.case_inputs(golden, case)
    fuser.set_tiles(lay)
    out = torch.zeros((1, H, W), dtype=torch.int16, device=DEV)
    coeffs = torch.zeros((1, lay.ntiles, 4), dtype=torch.float32, device=DEV)
    t_tiles = _dev(data)[None].contiguous()
    fuser.merge(_dev(emap)[None], t_tiles, out, zr, coeffs=coeffs)
    kap = F.tile_kappas(tiles, data, emap, zr)
    assert F.abcd_mismatch(coeffs.cpu().numpy()[0], golden[case + "_abcd"], kap) == []
    assert F.plane_mismatch(golden, case + "_out", _u16(out)[0]) == 0
    assert np.array_equal(t_tiles.cpu().numpy()[0], data), "merge must not modify the tiles"


@pytest.mark.parametrize("case", ["c1_256x128", "c1_200x100"])
def test_merge_batch3_golden_in_the_middle(fuser, golden, case):
    """pf_merge on a batch of 3: the recorded panorama at index 1 between two perturbed copies
    (another baseline, other tiles).  Index 1 equals the record, the neighbours do not.
    Engines: sweeps / streamed / resident at 256x128, sweeps / sweeps / streamed with partial
    patches at 200x100."""
    lay, tiles, data, emap, (W, H), zr = F.case_inputs(golden, case)
    fuser.set_tiles(lay)
    emaps = np.stack([emap * F.f32(0.8) + F.f32(0.1), emap, emap[::-1].copy()])
    datas = np.stack([F.f32(1) - data, data, np.roll(data, 977)])
    out = torch.zeros((3, H, W), dtype=torch.int16, device=DEV)
    coeffs = torch.zeros((3, lay.ntiles, 4), dtype=torch.float32, device=DEV)
    fuser.merge(_dev(emaps), _dev(datas), out, zr, coeffs=coeffs)
    got = _u16(out)
    kap = F.tile_kappas(tiles, data, emap, zr)
    assert F.abcd_mismatch(coeffs.cpu().numpy()[1], golden[case + "_abcd"], kap) == []
    assert np.array_equal(got[1], golden[case + "_out"])
    for b in (0, 2):
        assert (got[b] != golden[case + "_out"]).mean() > 0.5, b


def test_fuse_three_channel_baseline(fuser, golden):
    """pf_fuse with the 77 x 31 x 3 baseline (channel 0 is read, the width divides no level) on
    the untransformed tiles, the recorded coefficients applied on the fly.  Engines: sweeps /
    streamed / resident, packed."""
    case = "chan3_256x128"
    lay, tiles, data, emap, (W, H), zr = F.case_inputs(golden, case)
    assert emap.shape == (31, 77, 3)
    fuser.set_tiles(lay)
    out = torch.zeros((1, H, W), dtype=torch.int16, device=DEV)
    fuser.fuse(_dev(emap)[None], _dev(data)[None].contiguous(), out, zr,
               coeffs=_dev(golden[case + "_abcd"])[None])
    assert F.plane_mismatch(golden, case + "_out", _u16(out)[0]) == 0
    # channels 1 and 2 must not matter
    other = emap.copy()
    other[..., 1:] = F.f32(0.5)
    out2 = torch.zeros_like(out)
    fuser.fuse(_dev(other)[None], _dev(data)[None].contiguous(), out2, zr,
               coeffs=_dev(golden[case + "_abcd"])[None])
    assert torch.equal(out, out2)


def test_fuse_four_levels(fuser, golden):
    """pf_fuse at 4096 x 256: the four-level table, 200 / 150 / 100 / 50 sweeps at 512 / 1024 /
    2048 / 4096 wide.  Engines: resident (512 wide, a 25-row band) / streamed / streamed /
    streamed, packed."""
    case = "c1_4096x256"
    lay, tiles, data, emap, (W, H), zr = F.case_inputs(golden, case)
    assert panofuse.level_info(W, H, zr, 0)[5] == 4
    fuser.set_tiles(lay)
    out = torch.zeros((1, H, W), dtype=torch.int16, device=DEV)
    fuser.fuse(_dev(emap)[None], _dev(data)[None].contiguous(), out, zr)
    assert F.plane_mismatch(golden, case + "_out", _u16(out)[0]) == 0


@pytest.mark.parametrize("k", range(len(F.JOINT_SETS)))
def test_register_joint_lm(fuser, golden, k):
    """pf_register_joint under the LM solver against real Ceres on the same active set."""
    lay, tiles, data, emap, _, zr = F.case_inputs(golden, "c1_256x128")
    fuser.set_tiles(lay)
    c = torch.zeros((1, 4), dtype=torch.float32, device=DEV)
    fuser.register_joint(_dev(emap)[None], _dev(data)[None].contiguous(), zr, F.JOINT_SETS[k],
                         coeffs=c)
    got, ref = c.cpu().numpy()[0], golden[f"joint{k}_abcd"]
    rel = F.rel_diff(got, ref)
    print(f"joint {F.JOINT_SETS[k]}: rel {float(rel.max()):.3g}, "
          f"{int(F.ulp_diff(got, ref).max())} ulp")
    assert rel.max() <= F.ABCD_RTOL


@pytest.mark.parametrize("case", [c for c, v in F.CASES.items() if v[0] == "smooth"])
def test_solve_smoothing(fuser, golden, case):
    """pf_solve_smoothing at 256x128 and 200x100, a batch of 2 with the recorded tiles second."""
    lay, tiles, data, _, (W, H), zr = F.case_inputs(golden, case)
    fuser.set_tiles(lay)
    out = torch.zeros((2, H, W), dtype=torch.int16, device=DEV)
    fuser.solve_smoothing(_dev(np.stack([F.f32(1) - data, data])), out, zr)
    assert F.plane_mismatch(golden, case + "_out", _u16(out)[1]) == 0


@pytest.mark.parametrize("case", ["c1_256x128", "c1_200x100", "wide_256x128", "leres_512x256"])
def test_error_metrics_sequential(fuser, golden, case):
    """pf_error_metrics in the reference's summation order on the recorded result, the six
    (align_way, cap_depth) settings.  The band is the reference's global one (Depth.cpp:22,
    1983), in the wide-band case too."""
    _, _, out, _ = _register_and_fuse(fuser, golden, case)
    assert F.plane_mismatch(golden, case + "_out", out) == 0  # the recorded result itself
    gt = F.map_f32(golden["gt"])
    ref = golden[case + "_metrics"]
    fuser.set_metrics_order("sequential")
    try:
        for k, (aw, cap) in enumerate(F.SETTINGS):
            m = fuser.error_metrics(_dev(gt)[None], _dev(out.view(np.int16))[None], F.ZR, aw,
                                    bool(cap))[0]
            got = F.metric_bits(m, aw)
            exact = [i for i in range(8) if i != 3]
            assert np.array_equal(got[exact], ref[k][exact]), \
                (aw, cap, got.view(np.float32), ref[k].view(np.float32))
            a, b = float(got[3:4].view(np.float32)[0]), float(ref[k][3:4].view(np.float32)[0])
            assert a == b or abs(a - b) <= LOG_RTOL * abs(b), (aw, cap, a, b)
    finally:
        fuser.set_metrics_order("tree")
