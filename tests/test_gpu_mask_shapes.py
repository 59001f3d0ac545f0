"""The tile-pixel validity rule (pf_set_tile_validity) on the GPU beyond the one 512x256 C1 case of
tests/test_gpu_mask.py, bit for bit against the compositions of tests/mask_ref.py.

Under the rule the targets come from the MASK instantiations of targets_patch with per-panorama
counts, no level is packed or resident (every level runs the marker-reading general streamed
passes or the per-sweep kernel), the stitch walks boxes per pixel and the registration goes
through its *_valid kernels.  tests/mask_shapes.py has the cases -- seven output sizes that are no
powers of two, six hole sets placed on the fusion grid (a two-tile seam, the first and last band
rows, the first and last covered columns, a checkerboard across patch and strip borders, isolated
valid pixels, a whole tile), LeReS / MiDaS tiles with clamped taps, mixed off-grid tile sizes and
three channels -- and tests/test_mask_shapes.py proves them on the CPU.

Every comparison is array_equal on u16, or on fp32 / fp64 bit patterns with NaN where the
reference has NaN.  The CPU references are computed once per process (mask_shapes' caches); all
of them together take about 15 s, so no row of the table is dropped.  PF_JPLAN is read once per
process: one child process fuses every row with the rule on and its `jacobi plan` lines must name
`general C...` or `sweeps`, never `resident` or `packed`.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import mask_ref as M  # noqa: E402
import mask_shapes as MS  # noqa: E402
import panofuse  # noqa: E402
import pyoracle as O  # noqa: E402
import tile_shapes as TL  # noqa: E402
from test_gpu_fuse_shapes import PLAN  # noqa: E402
from test_gpu_mask import _dev, _same_bits  # noqa: E402

ZR = M.ZR
DEV = "cuda:0"
INF = float("inf")
SIZE_IDS = [MS.size_id(s) for s in MS.SIZES]
NBATCH = 9  # one more than kTNB, the targets kernel's panoramas per block
BATCH_SETS = ["seam", "bandrows", "edgecols", "none", "checker", "isolated", "tile", "bandrows",
              "checker"]
CHILD_SET = "seam"


class Fusers:
    """One context per layout and channel count, made on demand; `masked` switches the rule
    "finite values only" on, `clear` switches it off everywhere."""

    def __init__(self):
        self.made = {}

    def plain(self, case):
        key = (id(case.lay), case.channels)
        if key not in self.made:
            f = panofuse.Fuser(0)
            f.set_tiles(case.lay, channels=case.channels)
            self.made[key] = f
        return self.made[key]

    def masked(self, case):
        f = self.plain(case)
        f.set_tile_validity(-INF, INF)
        return f

    def clear(self):
        for f in self.made.values():
            f.set_tile_validity(None, None)


@pytest.fixture(scope="module")
def fusers():
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected on a host without a GPU")
    fz = Fusers()
    yield fz
    fz.clear()
    for f in fz.made.values():
        f.close()


@pytest.fixture()
def rule(fusers):
    """case -> its context with the rule on; the rule is off again after the test."""
    yield fusers.masked
    fusers.clear()


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


def _fuse(f, case, data, coeffs=None):
    """fuse() of data [B][tile_elems] on the case's baseline: u16 [B][out_h][out_w]."""
    data = np.atleast_2d(data)
    B = data.shape[0]
    out = torch.zeros((B, case.out_h, case.out_w), dtype=torch.int16, device=DEV)
    e = _dev(np.broadcast_to(case.emap, (B,) + case.emap.shape))
    f.fuse(e, _dev(data), out, ZR, coeffs=None if coeffs is None else _dev(coeffs))
    f.synchronize()
    return _u16(out)


def _differ(got, ref):
    assert got.shape == ref.shape and got.dtype == ref.dtype == np.uint16
    return int((got != ref).sum())


# ---- 1. fusion, every row x every hole set ------------------------------------------------------
@pytest.mark.parametrize("name", MS.SETS)
@pytest.mark.parametrize("size", MS.SIZES, ids=SIZE_IDS)
def test_fuse_rows(rule, size, name):
    case = MS.row_case(size)
    f = rule(case)
    ref, _ = MS.composition(case, name)
    raw, cf = MS.raw(case, name), MS.abcd(case)
    bad = _differ(_fuse(f, case, raw, cf[None])[0], ref)
    assert bad == 0, f"{case.name} {name}: {bad} pixels differ from the composition"
    assert np.count_nonzero(ref) > 0
    if size in MS.FULL_CHECKS:
        bad = _differ(_fuse(f, case, M.transform(case.tiles, raw, cf))[0], ref)
        assert bad == 0, f"{case.name} {name}: {bad} pixels differ (pre-transformed tiles)"
        out = torch.zeros((1, case.out_h, case.out_w), dtype=torch.int16, device=DEV)
        err = f.fuse_check(_dev(case.emap[None]), _dev(raw[None]), ZR, case.out_w,
                           out_h=case.out_h, coeffs=_dev(cf[None]), out=out)
        f.synchronize()
        bad = _differ(_u16(out)[0], ref)
        assert bad == 0, f"{case.name} {name}: {bad} pixels differ (fuse_check)"
        assert np.isfinite(err.cpu().numpy()).all()
    assert f.jres_errors() == 0


# ---- 2. the engine of every level under the rule, from a child's plan lines ---------------------
def _jobs():
    return [(s, CHILD_SET) for s in MS.SIZES] + [((1024, 400), "none")]


def _child(out_path):
    outs, errs = {}, []
    for k, (size, name) in enumerate(_jobs()):
        case = MS.row_case(size)
        f = panofuse.Fuser(0)
        try:
            f.set_tiles(case.lay)
            f.set_tile_validity(-INF, INF)
            outs[f"out{k}"] = _fuse(f, case, MS.raw(case, name), MS.abcd(case)[None])[0]
            errs.append(f.jres_errors())
        finally:
            f.close()
    np.savez(out_path, errs=np.array(errs, np.int64), **outs)


CHILD = ("import sys; sys.path[:0] = [{pkg!r}, {oracle!r}, {tests!r}]; "
         "import test_gpu_mask_shapes as t; t._child(sys.argv[1])")


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    """([u16 panorama], [jres errors], [[plan line fields per level]]) of _jobs(), PF_JPLAN=1."""
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected on a host without a GPU")
    out_path = tmp_path_factory.mktemp("mask_shapes") / "child.npz"
    here = os.path.dirname(os.path.abspath(__file__))
    code = CHILD.format(pkg=os.path.dirname(os.path.abspath(panofuse.__file__)),
                        oracle=os.path.dirname(os.path.abspath(O.__file__)), tests=here)
    env = dict(os.environ, PF_JPLAN="1")
    for k in ("PF_JSLOW", "PF_JRES", "PF_JACOBI", "PF_JRES_NB"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", code, str(out_path)], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stderr.splitlines() if ln.startswith("jacobi plan")]
    assert not [ln for ln in lines if "resident" in ln or "packed" in ln], lines
    plans = [PLAN.match(ln).groups() for ln in lines]
    jobs = _jobs()
    assert len(plans) == 3 * len(jobs), r.stderr[-3000:]
    z = np.load(out_path)
    return ([z[f"out{k}"] for k in range(len(jobs))], z["errs"].tolist(),
            [plans[3 * k:3 * k + 3] for k in range(len(jobs))])


def test_child_engines_and_outputs(child):
    outs, errs, plans = child
    seen = set()
    for k, (size, name) in enumerate(_jobs()):
        case = MS.row_case(size)
        tag = f"job {k} ({case.name} {name})"
        for level, (line, engine) in enumerate(zip(plans[k], MS.expected_engines(case))):
            lv = case.level(level)
            w, h, band, iters, batch, rest = line
            assert (int(w), int(h), int(band), int(iters), int(batch)) == \
                   (lv.w, lv.h, lv.h1 - lv.h0 + 1, lv.iters, 1), (tag, line)
            if engine == "sweeps":
                assert rest == "sweeps", (tag, level, line)
            else:
                assert rest.startswith("general C"), (tag, level, line)
            seen.add(engine)
        bad = _differ(outs[k], MS.composition(case, name)[0])
        assert bad == 0, f"{tag}: {bad} pixels differ from the composition"
        assert errs[k] == 0, tag
    assert seen == {"sweeps", "streamed"}
    # the rule on and nothing invalid, where the default path is resident: the oracle's panorama
    case = MS.row_case((1024, 400))
    d = M.transform(case.tiles, case.data, MS.abcd(case))
    ref, oops = O.solve_depth_all(case.emap, case.tiles, d, case.out_w, ZR, out_h=case.out_h)
    assert oops == 0 and _differ(outs[-1], ref) == 0


# ---- 3. batches ---------------------------------------------------------------------------------
@pytest.mark.parametrize("size", MS.BATCH_SIZES, ids=MS.size_id)
def test_batches(rule, size):
    """Batch 9: two groups of panoramas per block, the second partly filled (the bbeg + q < batch
    clamp), a different hole set per panorama and none in panorama 3, on partial patches."""
    case = MS.row_case(size)
    f = rule(case)
    assert len(BATCH_SETS) == NBATCH and BATCH_SETS[3] == "none"
    d = np.stack([MS.raw(case, n) for n in BATCH_SETS])
    cf = np.broadcast_to(MS.abcd(case), (NBATCH,) + MS.abcd(case).shape)
    got = _fuse(f, case, d, cf)
    for b in range(NBATCH):
        alone = _fuse(f, case, d[b], cf[b:b + 1])[0]
        bad = _differ(got[b], alone)
        assert bad == 0, f"{case.name} panorama {b}: {bad} pixels differ from its batch-1 result"
    for b in (0, 3, 8):
        bad = _differ(got[b], MS.composition(case, BATCH_SETS[b])[0])
        assert bad == 0, f"{case.name} panorama {b} ({BATCH_SETS[b]}): {bad} pixels differ"
    assert not np.array_equal(got[0], got[3]) and not np.array_equal(got[8], got[3])
    assert f.jres_errors() == 0


# ---- 4. other layouts ---------------------------------------------------------------------------
LAYOUT_SETS = ["seam", "checker", "isolated", "tile"]


def _merge_reference(case, d):
    """(coefficients fp32, u16): the masked registration, then the masked fusion under it (a tile
    with fewer than 4 valid samples has NaN coefficients and drops out)."""
    c64, _, _ = M.register(case.tiles, d, case.emap)
    c32 = c64.astype(np.float32)
    want, _ = M.masked_fuse(case.emap, case.tiles, M.transform(case.tiles, d, c32), case.out_w,
                            case.out_h, ZR)
    return c32, want


@pytest.mark.parametrize("layout", MS.LAYOUTS)
def test_layouts_fuse_and_merge(rule, layout):
    case = MS.layout_case(layout)
    f = rule(case)
    sets = LAYOUT_SETS + (["clamped"] if layout != "MIXED" else [])
    cf = MS.abcd(case)
    d = np.stack([MS.raw(case, n) for n in sets])
    got = _fuse(f, case, d, np.broadcast_to(cf, (len(sets),) + cf.shape))
    for b, name in enumerate(sets):
        bad = _differ(got[b], MS.composition(case, name)[0])
        assert bad == 0, f"{layout} {name}: {bad} pixels differ from the composition"
    # merge: the seam rectangle and a whole tile
    dm = M.apply_holes(case.tiles, case.data, MS.holes(case, "seam") + MS.holes(case, "tile"))
    c32, want = _merge_reference(case, dm)
    nt = len(case.tiles)
    assert np.isnan(c32[min(M.ALL_TILE, nt - 1)]).all() and np.isfinite(c32).all(1).sum() == nt - 1
    out = torch.zeros((1, case.out_h, case.out_w), dtype=torch.int16, device=DEV)
    gc = torch.zeros((1, nt, 4), dtype=torch.float32, device=DEV)
    t = _dev(dm[None])
    f.merge(_dev(case.emap[None]), t, out, ZR, coeffs=gc)
    f.synchronize()
    assert _same_bits(t.cpu().numpy()[0], dm), "merge must not modify tiles"
    assert _same_bits(gc.cpu().numpy()[0], c32)
    bad = _differ(_u16(out)[0], want)
    assert bad == 0, f"{layout} merge: {bad} pixels differ from the composition"
    assert f.jres_errors() == 0


@pytest.mark.parametrize("base", ["LERES", "MIDAS"])
def test_three_channels_equal_one(rule, base):
    """Three interleaved channels: the panorama of the one-channel tiles, and register(apply=True)
    writes channel 0 only -- the transform, NaN kept at invalid pixels -- and leaves -7 in 1-2."""
    c1, c3 = MS.layout_case(base), MS.layout_case(base + "3")
    got = {}
    for case in (c1, c3):
        f = rule(case)
        d = np.stack([MS.raw(case, "seam"), MS.raw(case, "clamped")])
        cf = MS.abcd(case)
        got[case.channels] = _fuse(f, case, d, np.broadcast_to(cf, (2,) + cf.shape))
    assert np.array_equal(got[1], got[3])
    assert np.array_equal(got[3][0], MS.composition(c3, "seam")[0])

    f = rule(c3)
    d = M.apply_holes(c3.tiles, c3.data, MS.holes(c3, "seam") + MS.holes(c3, "tile"))
    assert TL.fill_kept(d)
    c64, _, _ = M.register(c3.tiles, d, c3.emap)
    want = M.transform(c3.tiles, d, c64.astype(np.float32))
    t = _dev(d[None])
    gc = torch.zeros((1, len(c3.tiles), 4), dtype=torch.float32, device=DEV)
    f.register(_dev(c3.emap[None]), t, ZR, degree=3, apply=True, coeffs=gc)
    f.synchronize()
    x = t.cpu().numpy()[0]
    assert _same_bits(gc.cpu().numpy()[0], c64.astype(np.float32))
    assert TL.fill_kept(x), "register(apply) wrote a channel past the first"
    # NaN: every invalid pixel's channel 0, and the whole channel 0 of the all-invalid tile
    tl = c3.tiles[min(M.ALL_TILE, len(c3.tiles) - 1)]
    nan = np.isnan(d)
    nan[tl.offset:tl.offset + tl.width * tl.height * 3:3] = True
    assert np.array_equal(np.isnan(x), nan)
    assert _same_bits(x, want)


# ---- 5. registration on the mixed and three-channel layouts -------------------------------------
@pytest.mark.parametrize("layout", ["MIXED", "LERES3", "MIDAS3"])
def test_register_layouts(rule, layout):
    """An all-invalid tile, a tile left with exactly 3 valid samples (four NaNs) and one with
    exactly 4 (O.lm_moments' solution, or NaN where that is not finite), next to a clean panorama."""
    case = MS.layout_case(layout)
    f = rule(case)
    nt, ch = len(case.tiles), case.channels
    d = np.stack([M.apply_holes(case.tiles, case.data, MS.reg_holes(case)), np.array(case.data)])
    ref = [M.register(case.tiles, d[b], case.emap) for b in range(2)]
    e, three, four = (MS.REG_TILES[k] for k in ("empty", "three", "four"))
    assert (ref[0][2][e], ref[0][2][three], ref[0][2][four]) == (0, 3, 4)
    em, t = _dev(np.stack([case.emap, case.emap])), _dev(d)
    c32 = torch.zeros((2, nt, 4), dtype=torch.float32, device=DEV)
    c64 = torch.zeros((2, nt, 4), dtype=torch.float64, device=DEV)
    f.register(em, t, ZR, degree=3, apply=False, coeffs=c32, coeffs64=c64)
    counts = f.tile_valid_counts(em, t, ZR)
    j32 = torch.zeros((2, 4), dtype=torch.float32, device=DEV)
    j64 = torch.zeros((2, 4), dtype=torch.float64, device=DEV)
    f.register_joint(em, t, ZR, list(range(nt)), coeffs=j32, coeffs64=j64)
    f.synchronize()
    assert _same_bits(t.cpu().numpy(), d), "apply=0 wrote"
    g64, g32, cn = c64.cpu().numpy(), c32.cpu().numpy(), counts.cpu().numpy()
    for b in range(2):
        r64, sums, rcnt = ref[b]
        assert _same_bits(g64[b], r64), (b, g64[b], r64)
        assert _same_bits(g32[b], r64.astype(np.float32)), b
        assert np.array_equal(cn[b, :, 0], rcnt), b
        pixels = [int((~np.isnan(d[b][t_.offset:t_.offset + t_.width * t_.height * ch:ch])).sum())
                  for t_ in case.tiles]
        assert np.array_equal(cn[b, :, 1], pixels), b
        want = M.register_joint(sums, range(nt))
        assert np.isfinite(want).all()
        assert _same_bits(j64.cpu().numpy()[b], want), b
        assert _same_bits(j32.cpu().numpy()[b], want.astype(np.float32)), b
    assert np.isnan(g64[0, e]).all() and np.isnan(g64[0, three]).all()
    lm, _ = O.lm_moments(ref[0][1][four])
    assert _same_bits(g64[0, four], lm if np.isfinite(lm).all() else np.full(4, np.nan))
    assert np.isfinite(g64[1]).all()


# ---- 6. stitch ----------------------------------------------------------------------------------
STITCH_CASES = [("600x300", s) for s in MS.STITCH_SIZES] + [("LERES", (512, 256)),
                                                            ("LERES3", (512, 256)),
                                                            ("MIDAS3", (512, 256))]


@pytest.mark.parametrize("with_coeffs", [False, True], ids=["plain", "coeffs"])
@pytest.mark.parametrize("name,size", STITCH_CASES, ids=lambda v: v if isinstance(v, str)
                         else MS.size_id(v))
def test_stitch(rule, name, size, with_coeffs):
    """Batch 2 under the rule: a block of the first candidate tile and a pixel whose first two
    candidates are invalid and whose third is valid; a whole tile.  The pick itself is asserted
    on the CPU (test_mask_shapes)."""
    case = MS.row_case((600, 300)) if name == "600x300" else MS.layout_case(name)
    W, H = size
    f = rule(case)
    holes, third = MS.stitch_holes(case.tiles, W, H)
    assert third is not None
    d = np.stack([M.apply_holes(case.tiles, case.data, holes), MS.raw(case, "tile")])
    cf = MS.abcd(case)
    out = torch.full((2, H, W), -1, dtype=torch.int16, device=DEV)
    f.stitch(_dev(d), out,
             coeffs=_dev(np.broadcast_to(cf, (2,) + cf.shape)) if with_coeffs else None)
    f.synchronize()
    got = _u16(out)
    for b in range(2):
        want = M.stitch_valid(case.tiles, d[b], W, H, cf if with_coeffs else None)
        bad = _differ(got[b], want)
        assert bad == 0, f"{name} {W}x{H} panorama {b}: {bad} pixels differ"
    plain = M.stitch_valid(case.tiles, case.data, W, H, cf if with_coeffs else None)
    assert not np.array_equal(got[0], plain) and not np.array_equal(got[1], plain)


# ---- 7. refusals --------------------------------------------------------------------------------
def test_refusals_at_600x300(rule, fusers):
    case = MS.row_case((600, 300))
    f = rule(case)
    W, H = case.out_w, case.out_h
    e, t = _dev(case.emap[None]), _dev(case.data[None])
    out = torch.zeros((1, H, W), dtype=torch.int16, device=DEV)
    lv = case.level(2)
    a = torch.zeros((lv.h, lv.w), dtype=torch.float32, device=DEV)
    b = torch.zeros((lv.h, lv.w), dtype=torch.float32, device=DEV)
    calls = {
        "pf_fuse_partial": lambda: f.fuse_partial(t, None, 0, len(case.tiles), W, ZR, 2, a, b,
                                                  out_h=H),
        "pf_solve_smoothing": lambda: f.solve_smoothing(t, out, ZR),
        "pf_merge_disparity": lambda: f.merge_disparity(e, t, out, ZR),
    }
    for name, call in calls.items():
        with pytest.raises(panofuse.PanofuseError) as err:
            call()
        assert err.value.code == panofuse.PF_ESTATE, name
        assert "pf_set_tile_validity" in str(err.value) and name in str(err.value), name
    fusers.clear()
    for name, call in calls.items():  # and with the rule off they run
        call()
    f.synchronize()
