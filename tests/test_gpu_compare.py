"""GPU parity of the two-map comparison: pf_error_compare / pf_disp_depth_convert
(csrc/pf_compare.hip around the two pf_error_metrics calls) against the numpy restatement of
DepthNamespace::ErrorCompare (tests/compare_ref.py), which tests/test_compare_ref.py pins to the
reference's compiled code, and against the reference's own recorded floats and pixels
(tests/golden/compare_ref.npz).

Bars, sequential order (the reference's summation order): the final metrics under the bars of
tests/test_gpu_metrics.py for ErrorEmap (bit-exact; mselog within 1e-5 relative: the device's
log10f); fit_s, fit_o, vmin, vmax, n_nonblack bit-exact; the depth plane and the shifted plane
bit-exact.  Tree order: the planes, vmin / vmax and the u8 bit-exact against the restatement fed
the kernel's own fit (the fit is the metrics code's job there), the metrics under the tree-order
bars of tests/test_gpu_metrics.py.

The kernels handle 1024 units per block (256 threads x 4 vectors of 16 bytes, or x 4 pixels in the
scalar form), so 520 x 260 takes 33 vector blocks; 75 x 37 = 2775 pixels has a scalar tail, and in
a batch its panoramas start at element offsets 2775 and 5550, which are not 16-byte aligned."""
import math
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import compare_ref as R  # noqa: E402
import panofuse  # noqa: E402
import pf_layouts as PL  # noqa: E402
import pyoracle as O  # noqa: E402

ZR = PL.ZENITH_RANGE
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "compare_ref.npz")
LOG_RTOL = 1e-5   # tests/test_gpu_metrics.py
MEAN_RTOL = 1e-2  # tests/test_gpu_metrics.py, tree order
EXACT = ("n", "nlog", "delta1", "delta2", "delta3", "gt_median", "given_median", "median_shift")
MEANS = ("mse", "mae", "mre", "mselog")
NRUNS = 54


@pytest.fixture(scope="module")
def fuser():
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected on a host without a GPU")
    f = panofuse.Fuser(0)
    f.set_metrics_order("sequential")
    return f


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_metrics_exact(got, ref):
    """_check_exact of tests/test_gpu_metrics.py."""
    for k in EXACT + ("mse", "mae", "mre", "ls_s", "ls_o"):
        assert _same(got[k], ref[k]), (k, got[k], ref[k])
    assert _same(got["mselog"], ref["mselog"]) or \
        abs(got["mselog"] - ref["mselog"]) <= LOG_RTOL * abs(ref["mselog"]), \
        ("mselog", got["mselog"], ref["mselog"])


def _check_planes(got, depth, shifted, ref):
    for k in ("vmin", "vmax"):
        assert _same(got[k], ref[k]), (k, got[k], ref[k])
    assert got["n_nonblack"] == ref["n_nonblack"]
    assert np.array_equal(depth, ref["depth"], equal_nan=True)
    nn = ~np.isnan(ref["depth"])
    assert np.array_equal(_bits(depth)[nn], _bits(ref["depth"])[nn])  # -0.0 and 0.0 apart
    assert np.array_equal(shifted, ref["shifted"])


def _check_all(got, depth, shifted, ref):
    print({k: got[k] for k in ("mse", "mselog", "fit_s", "fit_o", "vmin", "vmax", "n_nonblack")})
    _check_metrics_exact(got, ref)
    for k in ("fit_s", "fit_o"):
        assert _same(got[k], ref[k]), (k, got[k], ref[k])
    _check_planes(got, depth, shifted, ref)


def _run(fuser, gt, given, disp, align=1, cap=True):
    """gt / given: one panorama or a batch (a leading axis when ndim says so)."""
    res, depth, shifted = fuser.compare(_dev(gt), _dev(given), ZR, disp, align, cap, planes=True)
    return res, depth.cpu().numpy(), shifted.cpu().numpy()


def scene(h, w):
    y, x = np.mgrid[0:h, 0:w]
    u, v = x / w, y / h
    s = 0.5 + 0.3 * np.sin(6.3 * u + 1.0) * np.cos(3.1 * v) + 0.15 * (u > 0.4) - 0.1 * (v > 0.6)
    return np.clip(s, 0.08, 1.0)


def make_pair(seed, gshape, vshape, spots=48, black=0.15, scale=1.0):
    """The golden's recipe: a gt with black pixels that reaches 1.0, and the disparity baseline
    0.03 / gt + 0.3 + noise, zero where its gt pixel is zero, with `spots` pixels around the
    disparity the fit maps to zero (negative or tiny s * v + o: black, or a depth above 10)."""
    rng = np.random.default_rng(seed)
    (gh, gw), (h, w) = gshape, vshape
    gt = scene(gh, gw).astype(np.float32)
    zero = rng.random((gh, gw)) < black
    gt[zero] = 0.0
    ys = (np.arange(h, dtype=np.float32) * (np.float32(gh) / np.float32(h))).astype(int)
    xs = (np.arange(w, dtype=np.float32) * (np.float32(gw) / np.float32(w))).astype(int)
    d = 0.03 / scene(h, w) + 0.3 + rng.normal(0, 0.001, (h, w))
    if spots:
        d.reshape(-1)[rng.choice(h * w, spots, replace=False)] = np.linspace(0.280, 0.300, spots)
    d[zero[np.ix_(ys, xs)]] = 0.0
    return gt, (d * scale).astype(np.float32)


def _channels(a, c, seed):
    """a as channel 0 of c interleaved channels, the others filled with other values."""
    rng = np.random.default_rng(seed)
    out = rng.uniform(0.1, 0.9, a.shape + (c,)).astype(np.float32)
    out[..., 0] = a
    return out


SHAPES = {
    "64x32": ((32, 64), (32, 64), 1, 1),
    "75x37": ((37, 75), (37, 75), 1, 1),          # odd: rows not 16-byte aligned, scalar tail
    "gt100x50-64x33": ((50, 100), (33, 64), 1, 1),
    "given_c3": ((32, 64), (32, 64), 1, 3),        # inverted three times, strided reads
    "given_c2": ((32, 64), (32, 64), 1, 2),        # inverted twice: almost the identity
    "gc3": ((32, 64), (32, 64), 3, 1),
    "520x260": ((260, 520), (260, 520), 1, 1),     # 33 blocks, two waves per row
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_disparity_chain(fuser, name):
    gshape, vshape, gc, vc = SHAPES[name]
    gt, given = make_pair(3, gshape, vshape)
    if gc > 1:
        gt = _channels(gt, gc, 4)
    if vc > 1:
        given = _channels(given, vc, 5)
    ref = R.compare(gt, given, ZR, True, 1, True)
    assert ref["fit_o"] < 0 and 0.05 < 1 - ref["n_nonblack"] / ref["depth"].size < 0.5
    res, depth, shifted = _run(fuser, gt[None], given[None], True)
    _check_all(res[0], depth[0], shifted[0], ref)


@pytest.mark.parametrize("align,cap", [(0, True), (2, False), (1, False)])
def test_disparity_align_and_cap(fuser, align, cap):
    gt, given = make_pair(6, (37, 75), (37, 75))
    ref = R.compare(gt, given, ZR, True, align, cap)
    res, depth, shifted = _run(fuser, gt[None], given[None], True, align, cap)
    _check_all(res[0], depth[0], shifted[0], ref)


def make_batch3():
    """Three 75 x 37 panoramas with three fits: [0] no cap pixels, its smallest depth planted at
    pixel 0 and its largest at the last pixel (rows outside the compared band, so the fit does
    not move); [1] black pixels, some from a negative s * v + o; [2] pixels at the cap."""
    shape = (37, 75)
    gt0, g0 = make_pair(11, shape, shape, spots=0, black=0.10)
    f = R.compare(gt0, g0, ZR, True, 1, True)
    s, o = np.float32(f["fit_s"]), np.float32(f["fit_o"])
    g0[0, 0] = np.float32((1.0 / 0.02 - o) / s)      # depth about 0.02: below every other
    g0[-1, -1] = np.float32((1.0 / 5.0 - o) / s)     # depth about 5: above every other
    gt1, g1 = make_pair(12, shape, shape, spots=48, black=0.25, scale=0.8)
    gt2, g2 = make_pair(13, shape, shape, spots=96, black=0.15, scale=1.1)
    gts, givens = np.stack([gt0, gt1, gt2]), np.stack([g0, g1, g2])
    refs = [R.compare(gts[b], givens[b], ZR, True, 1, True) for b in range(3)]
    return gts, givens, refs


@pytest.fixture(scope="module")
def batch3():
    return make_batch3()


def test_batch_of_three(fuser, batch3):
    gts, givens, refs = batch3
    # the conditions the case is there for, on the restatement
    assert len({(r["fit_s"], r["fit_o"]) for r in refs}) == 3
    d0 = refs[0]["depth"].reshape(-1)
    nb = ~(np.abs(d0).astype(np.float64) < 1e-4)
    assert np.flatnonzero(nb & (d0 == d0[nb].min())).tolist() == [0]
    assert np.flatnonzero(nb & (d0 == d0[nb].max())).tolist() == [d0.size - 1]
    assert refs[0]["vmin"] == float(d0[0]) and refs[0]["vmax"] == float(d0[-1]) < 10
    black1 = 1 - refs[1]["n_nonblack"] / d0.size
    assert 0.05 < black1 < 0.5
    sv = givens[1] * np.float32(refs[1]["fit_s"]) + np.float32(refs[1]["fit_o"])
    assert ((sv < 0) & (givens[1] != 0)).any()       # black from a negative s * v + o
    assert (refs[2]["depth"] == 10).any() and refs[2]["vmax"] == 10.0
    res, depth, shifted = _run(fuser, gts, givens, True)
    for b in range(3):
        _check_all(res[b], depth[b], shifted[b], refs[b])


def test_second_call_has_its_own_minmax(fuser, batch3):
    """Two calls on one context: the second panorama's range lies inside the first's, so cells
    left over from the first call would show in vmin / vmax."""
    gts, givens, refs = batch3
    gtb, gb = make_pair(14, (37, 75), (37, 75), spots=0, black=0.10)
    refb = R.compare(gtb, gb, ZR, True, 1, True)
    assert refs[0]["vmin"] < refb["vmin"] and refb["vmax"] < refs[0]["vmax"]
    assert refs[0]["n_nonblack"] != refb["n_nonblack"]
    res, depth, shifted = _run(fuser, gts[0:1], givens[0:1], True)
    _check_all(res[0], depth[0], shifted[0], refs[0])
    res, depth, shifted = _run(fuser, gtb[None], gb[None], True)
    _check_all(res[0], depth[0], shifted[0], refb)


@pytest.mark.parametrize("disp", [True, False])
def test_optional_planes(fuser, batch3, disp):
    """depth == NULL and / or shifted == NULL: the struct and the plane that is asked for do not
    change."""
    gts, givens, _ = batch3
    gt, given = _dev(gts), _dev(givens)
    full, depth, shifted = fuser.compare(gt, given, ZR, disp, 1, True, planes=True)
    for want_depth, want_shifted in ((False, True), (True, False), (False, False)):
        out = torch.zeros((3, panofuse.COMPARE_WORDS), dtype=torch.int32, device=DEV)
        d = torch.full_like(depth, -7.0) if want_depth else None
        s = torch.full_like(shifted, 99) if want_shifted else None
        fuser.compare_async(gt, given, ZR, out, disp, 1, True, d, s)
        fuser.synchronize()
        ref = torch.zeros_like(out)
        fuser.compare_async(gt, given, ZR, ref, disp, 1, True, depth.clone(), shifted.clone())
        fuser.synchronize()
        assert torch.equal(out, ref)
        if want_depth:
            assert torch.equal(d.view(torch.int32), depth.view(torch.int32))
        if want_shifted:
            assert torch.equal(s, shifted)
    assert full[0]["n"] > 0


@pytest.mark.parametrize("name", ["64x32", "75x37", "given_c3", "gt100x50-64x33"])
def test_depth_mode(fuser, name):
    gshape, vshape, gc, vc = SHAPES[name]
    gt, given = make_pair(7, gshape, vshape)
    given[0, :5] = [-0.5, 1.0, 1.5, 0.999, 0.0]   # below 0, at and above 1
    if vc > 1:
        given = _channels(given, vc, 8)
    ref = R.compare(gt, given, ZR, False, 1, True)
    res, depth, shifted = _run(fuser, gt[None], given[None], False)
    _check_all(res[0], depth[0], shifted[0], ref)
    assert res[0]["fit_s"] == 0 and res[0]["fit_o"] == 0 and res[0]["n_nonblack"] == 0
    assert res[0]["vmin"] == R.FLT_MAX and res[0]["vmax"] == -R.FLT_MAX
    em = fuser.error_metrics(_dev(gt[None]), _dev(given[None]), ZR, 1, True)[0]
    for k in em:
        assert _same(em[k], res[0][k]), (k, em[k], res[0][k])
    v0 = given[..., 0] if given.ndim == 3 else given
    assert np.array_equal(shifted[0], R.quantise(v0))
    assert shifted[0][0, :5].tolist() == [0, 255, 255, 254, 0]


def test_constant_given_plane(fuser):
    """det = 0 in the fit, so {s, o} are not finite: arithmetic only.  The planes, the u8 and the
    bounds equal the restatement fed the kernel's own {s, o}, NaN-aware; every pixel of a NaN
    plane is non-black, moves no bound and quantises to 0."""
    gt, _ = make_pair(9, (32, 64), (32, 64))
    given = np.full((32, 64), 0.5, np.float32)  # sums exact in float: det is exactly 0
    res, depth, shifted = _run(fuser, gt[None], given[None], True)
    got = res[0]
    print(got)
    assert not (math.isfinite(got["fit_s"]) and math.isfinite(got["fit_o"]))
    oracle = R.compare(gt, given, ZR, True, 1, True)
    assert not (math.isfinite(oracle["fit_s"]) and math.isfinite(oracle["fit_o"]))
    ref = R.compare(gt, given, ZR, True, 1, True, fit=(got["fit_s"], got["fit_o"]))
    _check_planes(got, depth[0], shifted[0], ref)
    if np.isnan(ref["depth"]).all():
        assert got["n_nonblack"] == given.size and not shifted.any()
        assert got["vmin"] == R.FLT_MAX and got["vmax"] == -R.FLT_MAX


def test_metrics_on_a_disparity_gt(fuser):
    """pf_error_metrics(align_way 2, no cap) alone on a gt in [1, 1e5], the range of a converted
    gt: the first ErrorEmap call of the chain."""
    rng = np.random.default_rng(21)
    gt = np.exp(rng.uniform(0.0, np.log(1e5), (2, 37, 75))).astype(np.float32)
    gt[rng.random(gt.shape) < 0.1] = 0.0
    gt[0, 20, 10], gt[1, 20, 11] = 1.0, 1e5
    given = (gt / np.float32(3e4) + rng.normal(0.3, 0.01, gt.shape)).astype(np.float32)
    got = fuser.error_metrics(_dev(gt), _dev(given), ZR, 2, False)
    for b in range(2):
        ref = O.error_metrics(gt[b], given[b], ZR, 2, False)
        print(got[b], ref)
        _check_metrics_exact(got[b], ref)


@pytest.mark.parametrize("channels", [1, 3])
def test_disp_depth_convert_in_place(fuser, channels):
    rng = np.random.default_rng(22)
    a = rng.uniform(-2, 2, (37, 75, channels)).astype(np.float32)
    a[0, :6, 0] = [0.0, 1e-5, 9.99e-6, -1.1e-5, np.float32(1e-5), -0.0]
    a[1, 0, 0] = np.nan
    want = a.copy()
    want[..., 0] = R.conv(a[..., 0], channels)
    t = _dev(a if channels > 1 else a[..., 0])
    fuser.disp_depth_convert(t, channels)
    fuser.synchronize()
    got = t.cpu().numpy().reshape(a.shape)
    nn = ~np.isnan(want)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(_bits(got)[nn], _bits(want)[nn])


@pytest.mark.parametrize("name", ["64x32", "75x37"])
def test_tree_order(fuser, name):
    gshape, vshape, _, _ = SHAPES[name]
    gt, given = make_pair(15, gshape, vshape)
    fuser.set_metrics_order("tree")
    try:
        res, depth, shifted = _run(fuser, gt[None], given[None], True)
    finally:
        fuser.set_metrics_order("sequential")
    got = res[0]
    ref = R.compare(gt, given, ZR, True, 1, True, fit=(got["fit_s"], got["fit_o"]))
    _check_planes(got, depth[0], shifted[0], ref)
    oracle = R.compare(gt, given, ZR, True, 1, True)
    for k in ("fit_s", "fit_o"):  # the fp64 tree against the reference's float sums
        assert abs(got[k] - oracle[k]) <= 5e-2 * max(1.0, abs(oracle[k])), (k, got[k], oracle[k])
    # _check(got, ref, 1) of tests/test_gpu_metrics.py
    for k in EXACT:
        assert _same(got[k], ref[k]), (k, got[k], ref[k])
    for k in MEANS:
        tol = MEAN_RTOL * abs(ref[k]) + 1e-9
        assert _same(got[k], ref[k]) or abs(got[k] - ref[k]) <= tol, (k, got[k], ref[k])


@pytest.fixture(scope="module")
def golden():
    return R.golden_cases(np.load(GOLDEN))


@pytest.mark.parametrize("k", range(NRUNS))
def test_golden_replay(fuser, golden, k):
    """Every recorded run at the C-ABI level against the reference's own floats and pixels."""
    c = golden[k]
    gt = R.load_map(c["gt_raw"], c["gt_kind"])
    given = R.load_map(c["given_raw"], c["given_kind"], True)
    res, _, shifted = _run(fuser, gt[None], given[None], c["disp"], c["align_way"], c["cap"])
    got = np.array([res[0][m] for m in R.METRICS], np.float32)
    print(c["id"], got, c["ref"])
    for i, m in enumerate(R.METRICS):
        a, b = float(got[i]), float(c["ref"][i])
        if m == "mselog":
            assert _same(a, b) or abs(a - b) <= LOG_RTOL * abs(b), (c["id"], m, a, b)
        else:
            assert _same(a, b), (c["id"], m, a, b)
    assert np.array_equal(shifted[0], c["pixels"]), c["id"]
