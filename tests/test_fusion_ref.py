"""The CPU oracle against the compiled reference on the registration / fusion / smoothing path.

tests/golden/fusion_ref.npz (tools/make_fusion_golden.py) records what the reference's own
SolveDepthToDepth (real Ceres 1.13), Depth2DepthTransform, SolveDepthAll, SolveDepthBySmoothing
and ErrorData return for the cases of tests/fusion_ref.py; every case ran under 1 and 4 OpenMP
threads with identical bits.  Here the oracle (oracle/pf_oracle.c, pf_oracle_lm.c) is held to the
record, with no reference tree at hand:

* per tile the coefficients of both LM forms (moment sums: the HIP kernel's form; sample-wise:
  Ceres' order) are the same bits on every well-conditioned tile and within 1e-5 relative on the
  ill-conditioned ones (fusion_ref.KAPPA_MAX says which, from the inputs alone);
* the transformed tiles agree on every bit and the fused / smoothed panoramas on every u16 (whole
  planes, or sha256 plus a strided subsample);
* the seven ErrorData floats of the six (align_way, cap_depth) settings are the same bits, and so
  is median_shift_factor where the reference writes it (align_way 1 only);
* joint registration over three active sets stays within 1e-5 relative in both forms;
* the oracle refuses output sizes whose levels do not double (4100x200, 502x251), where the
  reference's upsample reads past its previous level.

Measured when the fixture was made (the tool prints it): every coefficient of the well-conditioned
tiles 0 ulp in both forms; on the four degenerate tiles at most 24 ulp (moment form, 1.5e-6
relative) and 13 ulp (sample-wise); on the narrow-range LERES tiles at most 4 ulp.
"""
import functools
import os

import numpy as np
import pytest

import fusion_ref as F
import pyoracle as O
import test_fuse_shapes as TS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fusion_ref.npz")
LARGEST_FIXTURE = 542185  # tests/golden/large_merge.npz
MERGE = [c for c, v in F.CASES.items() if v[0] == "merge"]
FORMS = ("moments", "samples")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@functools.lru_cache(maxsize=None)
def _registered(case, form):
    """(abcd, transformed tile data, kappas) of a merge case by the oracle, computed once."""
    g = np.load(GOLDEN)
    lay, tiles, data, emap, size, zr = F.case_inputs(g, case)
    abcd, dt = F.oracle_register(tiles, data, emap, zr, form)
    return abcd, dt, F.tile_kappas(tiles, data, emap, zr)


def test_golden_covers_the_cases(golden):
    assert os.path.getsize(GOLDEN) <= LARGEST_FIXTURE
    cases = F.CASES
    sizes = {c: v[4] for c, v in cases.items()}
    # the C1 windows with 64 x 64 tiles, merged at three sizes, one with an odd level-0 width
    for c in ("c1_256x128", "c1_200x100", "c1_500x248"):
        assert cases[c][:4] == ("merge", "C1", (64, 64), "scene")
    assert sizes["c1_500x248"] == (500, 248) and O.level_dims(500, 248, F.ZR, 0).w % 2 == 1
    # a height that is not half the width
    assert any(v[0] == "merge" and v[4][1] != v[4][0] // 2 for v in cases.values())
    # the four-level iteration table, fusion only
    assert cases["c1_4096x256"][0] == "fuse" and O.num_levels(4096) == 4
    assert [O.level_dims(4096, 256, F.ZR, l).iters for l in range(4)] == [200, 150, 100, 50]
    # non-square tiles with the LERES windows
    assert cases["leres_512x256"][1:3] == ("LERES", (48, 40))
    assert golden["tiles_leres"].shape == (15, 40, 48)
    # a three-channel baseline whose size divides no level width
    b = golden[cases["chan3_256x128"][5]]
    assert b.ndim == 3 and b.shape[2] == 3
    assert all(O.level_dims(256, 128, F.ZR, l).w % b.shape[1] for l in range(3))
    # a second zenith band, wider than the default, the widest whole-degree one the oracle takes
    lay, tiles, data, emap, (W, H), zr = F.case_inputs(golden, "wide_256x128")
    assert zr[0] < F.ZR[0] and zr[1] > F.ZR[1] and zr == F.ZR_WIDE
    for lo, hi in ((5.0, 168.0), (6.0, 169.0), (3.0, 177.0)):
        with pytest.raises(ValueError, match=f"rc={O.EBAND}"):
            O.solve_depth_all(emap, tiles, data, W, (F.f32(F.PL.D2R(lo)), F.f32(F.PL.D2R(hi))),
                              out_h=H)
    assert float(lay.ranges[:, 2].min()) < F.ZR[0] and float(lay.ranges[:, 3].max()) > F.ZR[1]
    # clamps: exact 0 and 1 in every tile, both sample clamps and both output clamps fire
    t8 = golden["tiles_clamps"]
    assert all((t == 0).sum() > 100 and (t == 255).sum() > 100 for t in t8)
    lay, tiles, data, emap, _, zr = F.case_inputs(golden, "clamps_256x128")
    for p in range(lay.ntiles):
        xs, _, _, _ = O.reg_samples(tiles[p], data, emap, zr)
        assert (xs == 1e-4).any() and (xs == 1 - 1e-4).any(), p
    _, dt, _ = _registered("clamps_256x128", "moments")
    assert (dt == 0).any() and (dt == 1).any()
    # the five degenerate tiles
    d = golden["tiles_degenerate"]
    assert len(np.unique(d[0])) == 1 and d[0, 0, 0] not in (0, 255)
    assert len(np.unique(d[1])) == 2 and 0 not in d[1] and 255 not in d[1]
    assert not d[2].any()
    assert sorted(np.unique(d[3])) == [0, 255]
    assert not d[4][:, :32].any() and len(np.unique(d[4][:, 32:])) > 16
    assert len(F.DEGENERATE) == 5
    # joint registration sets, smoothing sizes
    assert F.JOINT_SETS == [[0, 2], [1, 3, 4], [0, 1, 2, 3, 4, 5]]
    assert all(f"joint{k}_abcd" in golden.files for k in range(3))
    assert {sizes[c] for c, v in cases.items() if v[0] == "smooth"} == {(256, 128), (200, 100)}
    # every case: the levels double, no tap index leaves its tile, the oops counts agree
    some_oops = 0
    for c, (mode, _, _, _, (W, H), _, zr) in cases.items():
        assert F.levels_double(W, H, zr), c
        assert c + "_out" in golden.files or c + "_out_sha256" in golden.files, c
        if mode == "smooth":
            continue
        lay, tiles, data, emap, _, _ = F.case_inputs(golden, c)
        if mode == "merge":
            data = _registered(c, "moments")[1]
        if (W, H) == (4096, 256):
            data = np.zeros_like(data)  # the counts do not depend on the values
        oops, oob = F.oracle_levels(tiles, data, W, H, zr)
        assert oob == 0, c
        assert oops == int(golden[c + "_oops"]), c
        some_oops += oops
    assert some_oops > 0
    # which tiles are ill-conditioned
    for c in MERGE:
        kap = _registered(c, "moments")[2]
        ill = tuple(p for p, k in enumerate(kap) if k > F.KAPPA_MAX)
        if c in F.SPLIT:
            assert ill
        else:
            assert ill == F.ILL_CONDITIONED.get(c, ()), (c, kap)


@pytest.mark.parametrize("case", sorted(F.ENGINES))
def test_engine_table(golden, case):
    """fusion_ref.ENGINES, which the GPU tests' docstrings cite, follows from the host's rules
    (tests/test_fuse_shapes.py: tcap, has_certificate, resident_blockings), and from
    expected_engines() itself where that applies: the default zenith range and no tap outside
    its tile's unit square."""
    lay, tiles, data, emap, (W, H), zr = F.case_inputs(golden, case)
    data = np.zeros_like(data)  # coverage does not depend on the values
    got = []
    for level in range(O.num_levels(W)):
        lv = O.level_dims(W, H, zr, level)
        _, cnt, _, _ = O.targets(tiles, data, lv)
        cert = TS.has_certificate(cnt, lv)
        engine = "sweeps" if TS.tcap(lv) < 1 else \
            "resident" if cert and TS.resident_blockings(lv) else "streamed"
        got.append((engine, "packed" if cert else "general", "partial" if lv.w % 64 else "full"))
    assert tuple(got) == F.ENGINES[case]
    if zr == F.ZR and int(golden[case + "_oops"]) == 0:
        assert TS.expected_engines(tiles, data, W, H) == [g[:2] for g in got]


def test_engine_table_reaches_every_engine():
    """Together the cases take every engine, both forms and both kinds of target patch; the
    per-sweep kernel, the general form and the partial patches are what the C1 / C2 parity tests
    (512- and 2048-wide outputs, default band) never reach."""
    cells = {c for rows in F.ENGINES.values() for c in rows}
    assert {c[0] for c in cells} == {"sweeps", "streamed", "resident"}
    assert {c[1] for c in cells} == {"packed", "general"}
    assert {c[2] for c in cells} == {"full", "partial"}
    assert set(F.ENGINES) == {c for c, v in F.CASES.items() if v[0] != "smooth"}


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", MERGE)
def test_registration_and_transform(golden, case, form):
    """SolveDepthToDepth per tile with only that tile active, then Depth2DepthTransform."""
    abcd, dt, kap = _registered(case, form)
    ref = golden[case + "_abcd"]
    print(f"{case} {form}: abcd up to {int(F.ulp_diff(abcd, ref).max())} ulp, rel "
          f"{float(F.rel_diff(abcd, ref).max()):.3g}; kappa {min(kap):.3g} .. {max(kap):.3g}")
    assert F.abcd_mismatch(abcd, ref, kap, case in F.SPLIT) == []
    lay, tiles, data, emap, _, zr = F.case_inputs(golden, case)
    if case in F.SPLIT:  # the transform from the recorded coefficients (fusion_ref.SPLIT)
        dt = data.copy()
        for p in range(lay.ntiles):
            O.depth_to_depth(tiles[p], dt, ref[p])
    n, (tw, th) = lay.ntiles, F.CASES[case][2]
    assert F.plane_mismatch(golden, case + "_tiles", F.bits(dt).reshape(n, th, tw)) == 0


@functools.lru_cache(maxsize=None)
def _fused(case, form):
    g = np.load(GOLDEN)
    lay, tiles, data, emap, (W, H), zr = F.case_inputs(g, case)
    if F.CASES[case][0] == "merge":
        data = _registered(case, form)[1]
        if case in F.SPLIT:
            data = F.case_inputs(g, case)[2].copy()
            for p in range(lay.ntiles):
                O.depth_to_depth(tiles[p], data, g[case + "_abcd"][p])
    out, oops = O.solve_depth_all(emap, tiles, data, W, zr, out_h=H)
    return out, oops


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", MERGE)
def test_solve_depth_all_after_registration(golden, case, form):
    out, oops = _fused(case, form)
    assert oops == int(golden[case + "_oops"])
    assert F.plane_mismatch(golden, case + "_out", out) == 0
    assert np.count_nonzero(out) > out.size // 2


@pytest.mark.parametrize("case", [c for c in MERGE if F.CASES[c][4][1] == F.CASES[c][4][0] // 2
                                  and c not in F.SPLIT])
def test_merge_entry_points(golden, case):
    """pfo_merge (moment form) and pfo_merge_lm (sample-wise), the calls the GPU parity tests
    use, on the cases whose height is half the width."""
    lay, tiles, data, emap, (W, H), zr = F.case_inputs(golden, case)
    kap = _registered(case, "moments")[2]
    for fn in (O.merge, O.merge_lm):
        d = data.copy()
        out, abcd = fn(emap, tiles, d, W, zr)
        assert F.abcd_mismatch(abcd, golden[case + "_abcd"], kap) == []
        assert F.plane_mismatch(golden, case + "_out", out) == 0
        n, (tw, th) = lay.ntiles, F.CASES[case][2]
        assert F.plane_mismatch(golden, case + "_tiles", F.bits(d).reshape(n, th, tw)) == 0


def test_fuse_only_four_levels(golden):
    """SolveDepthAll on untransformed tiles at 4096 x 256: levels 512 / 1024 / 2048 / 4096 with
    200 / 150 / 100 / 50 sweeps."""
    out, oops = _fused("c1_4096x256", "moments")
    assert oops == 0 == int(golden["c1_4096x256_oops"])
    assert F.plane_mismatch(golden, "c1_4096x256_out", out) == 0


@pytest.mark.parametrize("case", [c for c, v in F.CASES.items() if v[0] == "smooth"])
def test_solve_smoothing(golden, case):
    lay, tiles, data, _, (W, H), zr = F.case_inputs(golden, case)
    out = O.solve_smoothing(tiles, data, W, H, zr)
    assert F.plane_mismatch(golden, case + "_out", out) == 0
    assert np.count_nonzero(out) > W


@pytest.mark.parametrize("k", range(len(F.JOINT_SETS)))
def test_joint_registration(golden, k):
    """SolveDepthToDepth with several active maps: the samples of every active tile in one
    problem, in tile order.  Both LM forms within 1e-5 relative of real Ceres."""
    lay, tiles, data, emap, _, zr = F.case_inputs(golden, "c1_256x128")
    xs, ys = F.joint_samples(tiles, data, emap, zr, F.JOINT_SETS[k])
    ref = golden[f"joint{k}_abcd"]
    c, s = O.lm_fit(xs, ys)
    assert s["termination"] == "function_tolerance"
    X2, X3 = xs * xs, xs * xs * xs
    S = np.array([np.sum(X3 * X3), np.sum(X3 * X2), np.sum(X3 * xs), np.sum(X3), np.sum(X2 * X2),
                  np.sum(X2 * xs), np.sum(X2), np.sum(xs * xs), np.sum(xs), float(xs.size),
                  np.sum(X3 * ys), np.sum(X2 * ys), np.sum(xs * ys), np.sum(ys), np.sum(ys * ys)])
    cm, _ = O.lm_moments(S)
    for name, got in (("sample-wise", c), ("moments", cm)):
        rel = F.rel_diff(got.astype(np.float32), ref)
        print(f"joint {F.JOINT_SETS[k]} {name}: rel {float(rel.max()):.3g}, "
              f"{int(F.ulp_diff(got.astype(np.float32), ref).max())} ulp")
        assert rel.max() <= F.ABCD_RTOL, name


@pytest.mark.parametrize("case", MERGE)
def test_error_data(golden, case):
    """ErrorData on the recorded result.  The reference takes its band from the global
    g_zenith_range (Depth.cpp:22, 1983), not from the range the fusion ran with, so the oracle is
    given the default range in the wide-band case too."""
    out, _ = _fused(case, "moments")
    gt = F.map_f32(golden["gt"])
    assert gt.shape == F.GT_SHAPE and (gt[20:27, 30:44] == 0).all()
    ref = golden[case + "_metrics"]
    for k, (aw, cap) in enumerate(F.SETTINGS):
        m = O.error_metrics(gt, out, F.ZR, aw, bool(cap))
        assert m["n"] > 0 and m["nlog"] > 0
        got = F.metric_bits(m, aw)
        assert np.array_equal(got, ref[k]), (aw, cap, got.view(np.float32), ref[k].view(np.float32))
        assert (ref[k, 7] == F.UNSET_BITS) == (aw != 1)


@pytest.mark.parametrize("W,H,dims", [(4100, 200, (512, 1025, 2050, 4100)),
                                      (502, 251, (125, 251, 502))])
def test_oracle_refuses_levels_that_do_not_double(golden, W, H, dims):
    """The reference's upsample reads buffer_prev[(y / 2) * (width / 2) + x / 2]: at 4100 x 200
    x / 2 reaches 512 in a 512-wide row and the last row reads past the buffer.  The library
    refuses such sizes (prepare_levels); so does the oracle, before it touches a buffer."""
    assert tuple(O.level_dims(W, H, F.ZR, l).w for l in range(len(dims))) == dims
    assert not F.levels_double(W, H, F.ZR)
    lay, tiles, data, emap, _, _ = F.case_inputs(golden, "c1_256x128")
    with pytest.raises(ValueError, match=f"rc={O.ELEVELS}"):
        O.solve_depth_all(emap, tiles, data, W, F.ZR, out_h=H)
    with pytest.raises(ValueError):
        O.merge(emap, tiles, data.copy(), 502, F.ZR)
