"""The argument checks that open the C-ABI entry points, and the level cache behind them.

Every fusion-level entry point runs the same prologue (context and layout checks, the level cache
of prepare_levels, the level-range check, then its own buffer / tile-range / row-range checks) and
the evaluation entries share a shorter one.  test_single_fault_errors_unchanged pins the error code
and the full pf_last_error text of calls with exactly one bad argument, so that the order and the
wording of those checks stay what callers have seen so far.  No case reaches a kernel: each call
fails in its checks.

test_failed_level_rebuild_invalidates_cache covers prepare_levels itself: a rebuild that fails
after level 0 was rewritten must leave the cache invalid, so the next call with the old size
rebuilds it instead of running on the failed size's level dimensions.

All at the suite's smallest config: C1 (6 tiles of 256^2), output 512x256, baseline 128 wide,
batch 1.
"""
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import panofuse  # noqa: E402
import pf_layouts as PL  # noqa: E402
import pf_synth  # noqa: E402

ZR = PL.ZENITH_RANGE
DEV = "cuda:0"
OUT_W, EW = PL.CONFIGS["C1"]
OUT_H = OUT_W // 2
Z0, Z1 = float(ZR[0]), float(ZR[1])


def _fuser():
    lay = PL.config_layout("C1")
    fz = panofuse.Fuser(0)
    fz.set_tiles(lay)
    return fz, lay


def _error_of(call):
    """(code, message) of the PanofuseError the call raises, or None if it returns."""
    try:
        call()
    except panofuse.PanofuseError as e:
        return e.code, str(e)
    return None


def _raw(fz, name, *args):
    """A call through the ctypes handle (for NULL buffers and for entry points whose Fuser
    method checks the level on the host first); raises as Fuser._check does."""
    def call():
        fz._check(getattr(fz.L, name)(fz.h, *args))
    return call


def test_single_fault_errors_unchanged():
    fz, lay = _fuser()
    n = lay.ntiles
    nlev = panofuse.level_info(OUT_W, OUT_H, ZR, 0)[5]
    h_l0 = panofuse.level_info(OUT_W, OUT_H, ZR, 0)[1]
    assert (n, nlev, h_l0) == (6, 3, 64)
    f32 = [torch.zeros(OUT_W * OUT_H, dtype=torch.float32, device=DEV) for _ in range(4)]
    a, b, c, d = f32
    u16 = torch.zeros(OUT_W * OUT_H, dtype=torch.int16, device=DEV)
    taps = torch.zeros(OUT_W * OUT_H * 5, dtype=torch.int32, device=DEV)
    tiles = torch.zeros((1, fz.tile_elems), dtype=torch.float32, device=DEV)
    coeffs = torch.zeros((1, n, 4), dtype=torch.float32, device=DEV)
    emap = torch.ones((1, EW // 2, EW), dtype=torch.float32, device=DEV)
    P = panofuse._ptr
    size = (OUT_W, OUT_H, Z0, Z1)

    cases = []  # (name, call, expected message or None for "returns")
    for lv in (nlev, -1):
        bad = f"bad level {lv}"
        cases += [
            (f"fuse_partial level {lv}",
             lambda lv=lv: fz.fuse_partial(tiles, coeffs, 0, n, OUT_W, ZR, lv, a, b), bad),
            (f"fuse_partial_rows level {lv}",
             lambda lv=lv: fz.fuse_partial_rows(tiles, coeffs, 0, n, OUT_W, ZR, lv, 0, 1, a, b), bad),
            (f"fuse_coverage_rows level {lv}",
             lambda lv=lv: fz.fuse_coverage_rows(OUT_W, ZR, lv, 0, 1, a), bad),
            (f"fuse_normalize_rows level {lv}",
             lambda lv=lv: fz.fuse_normalize_rows(a, b, OUT_W, ZR, lv, 0, 1, c), bad),
            (f"fuse_tile_rows level {lv}",
             lambda lv=lv: fz.fuse_tile_rows(OUT_W, ZR, lv, 0, n), bad),
            (f"fuse_seed level {lv}",
             lambda lv=lv: fz.fuse_seed(emap, a, OUT_W, ZR, lv, b), bad),
            (f"fuse_finish_level level {lv}",
             lambda lv=lv: fz.fuse_finish_level(a, b, OUT_W, ZR, lv, c), bad),
            (f"fuse_level level {lv}",
             lambda lv=lv: fz.fuse_level(emap, a, b, c, OUT_W, ZR, lv, d), bad),
            (f"fuse_targets level {lv}",
             lambda lv=lv: fz.fuse_targets(tiles, coeffs, OUT_W, ZR, lv, a), bad),
            (f"fuse_normalize level {lv}",
             lambda lv=lv: fz.fuse_normalize(a, b, OUT_W, ZR, lv, c), bad),
            (f"multicover level {lv}",
             lambda lv=lv: fz.multicover(tiles, coeffs, 0, n, OUT_W, ZR, lv, a), bad),
            (f"multicover_patch level {lv}",
             lambda lv=lv: fz.multicover_patch(OUT_W, ZR, lv, a, b), bad),
            (f"fuse_border level {lv}",
             lambda lv=lv: fz.fuse_border(a, OUT_W, ZR, lv, a=b, b=c, out=u16), bad),
            (f"fuse_band_plan level {lv}",
             lambda lv=lv: fz.fuse_band_plan(OUT_W, ZR, lv, 2), bad),
            (f"fuse_band_pass level {lv}",
             lambda lv=lv: fz.fuse_band_pass(a, 0, OUT_W, ZR, lv, 1, 0, 1, src=b, dst=c), bad),
            # Fuser.probe_taps asks pf_level_info for the level's size first: the raw entry
            (f"probe_taps level {lv}", _raw(fz, "pf_probe_taps", *size, lv, P(taps)), bad),
        ]
    # the multi-cover entry checks its tile range only on a level that has pixels covered by three
    # or more tiles (it returns before that otherwise); the first such level, if the layout has one
    mc_level = next((lv for lv in range(nlev) if fz.multicover_count(OUT_W, ZR, lv) > 0), None)
    for t0, t1 in ((0, n + 1), (2, 1)):
        bad = f"tile range [{t0},{t1}) outside [0,{n})"
        cases += [
            (f"fuse_partial tiles [{t0},{t1})",
             lambda t0=t0, t1=t1: fz.fuse_partial(tiles, coeffs, t0, t1, OUT_W, ZR, 0, a, b), bad),
            (f"fuse_partial_rows tiles [{t0},{t1})",
             lambda t0=t0, t1=t1: fz.fuse_partial_rows(tiles, coeffs, t0, t1, OUT_W, ZR, 0, 0, 1,
                                                       a, b), bad),
            (f"fuse_tile_rows tiles [{t0},{t1})",
             lambda t0=t0, t1=t1: fz.fuse_tile_rows(OUT_W, ZR, 0, t0, t1), bad),
            (f"multicover tiles [{t0},{t1})",
             lambda t0=t0, t1=t1: fz.multicover(tiles, coeffs, t0, t1, OUT_W, ZR,
                                                0 if mc_level is None else mc_level, a),
             None if mc_level is None else bad),
        ]
    bad = f"rows [0,{h_l0 + 1}) outside [0,{h_l0})"
    cases += [
        ("fuse_partial_rows rows",
         lambda: fz.fuse_partial_rows(tiles, coeffs, 0, n, OUT_W, ZR, 0, 0, h_l0 + 1, a, b), bad),
        ("fuse_coverage_rows rows",
         lambda: fz.fuse_coverage_rows(OUT_W, ZR, 0, 0, h_l0 + 1, a), bad),
        ("fuse_normalize_rows rows",
         lambda: fz.fuse_normalize_rows(a, b, OUT_W, ZR, 0, 0, h_l0 + 1, c), bad),
    ]
    gt = torch.ones((1, OUT_H, OUT_W), dtype=torch.float32, device=DEV)
    cases += [
        ("error_metrics align_way", lambda: fz.error_metrics(gt, gt.clone(), ZR, align_way=3),
         "align_way 3"),
        ("compare align_way", lambda: fz.compare(gt, gt.clone(), ZR, False, align_way=3),
         "align_way 3"),
    ]
    # one NULL buffer each, on entries whose NULL check comes before any launch
    nb = "NULL buffer"
    ymin = panofuse.C.c_int()
    cases += [
        ("fuse_partial NULL lsum",
         _raw(fz, "pf_fuse_partial", P(tiles), P(coeffs), 0, n, *size, 0, None, P(b)), nb),
        ("fuse_partial_rows NULL cnt",
         _raw(fz, "pf_fuse_partial_rows", P(tiles), P(coeffs), 0, n, *size, 0, 0, 1, P(a), None),
         nb),
        ("fuse_coverage_rows NULL cnt", _raw(fz, "pf_fuse_coverage_rows", *size, 0, 0, 1, None), nb),
        ("fuse_normalize_rows NULL lnorm",
         _raw(fz, "pf_fuse_normalize_rows", P(a), P(b), *size, 0, 0, 1, None), nb),
        ("fuse_tile_rows NULL ymax",
         _raw(fz, "pf_fuse_tile_rows", *size, 0, 0, n, panofuse.C.byref(ymin), None),
         "NULL output"),
        ("fuse_seed NULL buf", _raw(fz, "pf_fuse_seed", P(emap), EW, EW // 2, 1, None, *size, 0, None),
         nb),
        ("fuse_seed NULL prev", _raw(fz, "pf_fuse_seed", None, 0, 0, 0, None, *size, 1, P(b)),
         "level 1 needs the previous level's buffer"),
        ("fuse_finish_level NULL cnt",
         _raw(fz, "pf_fuse_finish_level", P(a), None, *size, 0, P(c), None), nb),
        ("fuse_level NULL buf",
         _raw(fz, "pf_fuse_level", P(emap), EW, EW // 2, 1, None, P(a), P(b), *size, 0, None, None),
         nb),
        ("fuse_level NULL prev",
         _raw(fz, "pf_fuse_level", None, 0, 0, 0, None, P(a), P(b), *size, 1, P(c), None),
         "level 1 needs the previous level's buffer"),
        ("fuse_targets NULL lnorm",
         _raw(fz, "pf_fuse_targets", P(tiles), P(coeffs), *size, 0, None), nb),
        ("fuse_normalize NULL lnorm", _raw(fz, "pf_fuse_normalize", P(a), P(b), *size, 0, None), nb),
        ("fuse_border NULL prev",
         _raw(fz, "pf_fuse_border", None, *size, 1, P(a), P(b), None),
         "level 1 needs the previous level"),
        ("fuse_border NULL out", _raw(fz, "pf_fuse_border", P(a), *size, nlev - 1, P(b), P(c), None),
         nb),
        ("fuse_band_pass NULL lnorm",
         _raw(fz, "pf_fuse_band_pass", None, 0, 0, 0, None, None, 0, P(a), P(b), None, *size, 1, 1,
              0, 1), nb),
        ("probe_taps NULL", _raw(fz, "pf_probe_taps", *size, 0, None), nb),
    ]

    got = {name: _error_of(call) for name, call, _ in cases}
    torch.cuda.synchronize()
    want = {name: None if msg is None else (panofuse.PF_EINVAL, f"panofuse error -1: {msg}")
            for name, _, msg in cases}
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong
    fz.close()


def test_failed_level_rebuild_invalidates_cache():
    fz, lay = _fuser()
    n = lay.ntiles
    nlev = panofuse.level_info(OUT_W, OUT_H, ZR, 0)[5]
    seeds = pf_synth.seeds_for(1, 20261019)
    gt = pf_synth.scene_depth(seeds, OUT_W, OUT_H, DEV).contiguous()
    emap = pf_synth.baseline_emap(seeds, EW, EW // 2, DEV).contiguous()
    tiles = torch.zeros((1, fz.tile_elems), dtype=torch.float32, device=DEV)
    fz.warp_depth(gt, tiles, panofuse.make_responses(pf_synth.responses(seeds, n), DEV))
    coeffs = torch.zeros((1, n, 4), dtype=torch.float32, device=DEV)
    fz.register(emap, tiles, ZR, apply=False, coeffs=coeffs)

    def fuse():
        out = torch.zeros((1, OUT_H, OUT_W), dtype=torch.int16, device=DEV)
        fz.fuse(emap, tiles, out, ZR, coeffs=coeffs)
        fz.synchronize()
        return out.cpu()

    def queries():
        res = []
        for lv in range(nlev):
            res.append(fz.fuse_tile_rows(OUT_W, ZR, lv, 0, n))
            try:  # defined where the zenith band leaves room for streaming passes
                res.append(fz.fuse_band_plan(OUT_W, ZR, lv, 2))
            except panofuse.PanofuseError as e:
                res.append(str(e))
        return res

    first = fuse()
    before = queries()
    assert any(isinstance(r, list) and r for r in before), before
    # 1028x514: level 0 is 257x128 and level 1 is 514x257, and 257 is not twice 128, so the
    # rebuild fails at level 1, after level 0 of the cache was rewritten
    bad_w = 1028
    assert panofuse.level_info(bad_w, bad_w // 2, ZR, 0)[:2] == (257, 128)
    assert panofuse.level_info(bad_w, bad_w // 2, ZR, 1)[:2] == (514, 257)
    with pytest.raises(panofuse.PanofuseError) as ei:
        fz.fuse_tile_rows(bad_w, ZR, 0, 0, n)
    assert ei.value.code == panofuse.PF_EINVAL
    assert str(ei.value) == "panofuse error -1: output 1028x514 is not divisible by 2^2"
    assert queries() == before
    # only now a fusion: its level dimensions are those the queries just showed
    assert torch.equal(fuse(), first)
    fz.close()
