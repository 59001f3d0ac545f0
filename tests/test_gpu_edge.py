"""GPU parity of the edge-fidelity metrics: pf_error_laplacian (csrc/pf_edge.hip) against the
numpy fp64 restatement of DepthNamespace::ErrorLaplacian (tests/edge_ref.py), which itself is
pinned to the reference's compiled code by tests/golden/edge_metrics_ref.npz
(tests/test_edge_ref.py).

Bars: the three sample counts equal; the three maps (gt Laplacian, given Laplacian, absolute
error) bit-identical, since every per-pixel term is the same fp64 expression of the same taps; the
five means within 2 * N * 2^-53 relative of the exact (math.fsum) mean, N = w * h: any summation
order of N non-negative fp64 terms is within (N - 1) * 2^-53 of the exact sum, the factor 2
covers the final divide.  That is 2.3e-10 at 2048 x 1024 and 4.5e-13 at 64 x 32.

The kernel works on tiles of TILE_X x TILE_Y given-map pixels per block; a thread walks down
TILE_Y / 2 rows of one column."""
import math
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import edge_ref as E  # noqa: E402
import panofuse  # noqa: E402
import pf_layouts as PL  # noqa: E402
import pf_synth  # noqa: E402
import pyoracle as O  # noqa: E402

DEV = "cuda:0"
TILE_X, TILE_Y = 128, 32  # EDGE_TILE_X / EDGE_TILE_Y of csrc/pf_internal.hpp
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "edge_metrics_ref.npz")


@pytest.fixture(scope="module")
def fuser():
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected on a host without a GPU")
    return panofuse.Fuser(0)


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).to(DEV)


def _maps(h, w, gh=None, gw=None, seed=0, zeros=0.03):
    """A gt [gh][gw] in (0.05, 0.95) with a fraction of zero pixels, and a float given [h][w]."""
    rng = np.random.default_rng(seed)
    gh, gw = gh or h, gw or w
    gt = rng.uniform(0.05, 0.95, (gh, gw)).astype(np.float32)
    gt[rng.random((gh, gw)) < zeros] = 0.0
    given = rng.uniform(0.0, 1.0, (h, w)).astype(np.float32)
    return gt, given


def _check(got, ref, w, h):
    for k in E.COUNTS:
        assert got[k] == ref[k], (k, got[k], ref[k])
    for k in E.KEYS:
        print(k, got[k], ref[k], E.mean_bound(w, h))
        assert E.close(got[k], ref[k], w, h), (k, got[k], ref[k], E.mean_bound(w, h))


def _run_check(fuser, gt, given, gt_ch0=None, given_ch0=None):
    """One panorama through the GPU with maps, against the restatement of channel 0."""
    g0 = gt if gt_ch0 is None else gt_ch0
    v0 = given if given_ch0 is None else given_ch0
    if v0.dtype == np.uint16:
        v0 = E.u16_to_float(v0)
    h, w = v0.shape
    ref, rmaps = E.edge_metrics(g0, v0, maps=True)
    res, gl, vl, ae = fuser.edge_metrics(_dev(gt[None]), _dev(given[None]), maps=True)
    _check(res[0], ref, w, h)
    for name, t in (("gt_lap", gl), ("given_lap", vl), ("lap_ae", ae)):
        assert t.dtype == torch.float64 and tuple(t.shape) == (1, h, w)
        assert np.array_equal(t.cpu().numpy()[0], rmaps[name]), name
    return res[0], ref


@pytest.mark.parametrize("k", range(5))
def test_golden_pairs(fuser, k):
    """The recorded pairs: against the restatement and directly against the reference's doubles."""
    z = np.load(GOLDEN)
    g16, v16, ref, counts = z[f"gt{k}"], z[f"given{k}"], z[f"ref{k}"], z[f"counts{k}"]
    got, _ = _run_check(fuser, E.u16_to_float(g16), v16)
    h, w = v16.shape
    assert [got[c] for c in E.COUNTS] == counts.tolist()
    for i, key in enumerate(E.KEYS):
        assert E.close(got[key], float(ref[i]), w, h), (key, got[key], float(ref[i]))


def test_smallest_5x5(fuser):
    gt, given = _maps(5, 5, seed=1, zeros=0.0)
    got, _ = _run_check(fuser, gt, given)
    assert (got["n_lap5"], got["n_lap"], got["n_sobel"]) == (1, 9, 9)


def test_smallest_4x4(fuser):
    gt, given = _maps(4, 4, seed=2, zeros=0.0)
    got, _ = _run_check(fuser, gt, given)
    assert got["n_lap5"] == 0 and math.isnan(got["lap5_mae"])
    assert got["n_lap"] == 4 and got["n_sobel"] == 4
    assert all(math.isfinite(got[k]) for k in E.KEYS[:4])


def test_smallest_2x2(fuser):
    gt, given = _maps(2, 2, seed=3, zeros=0.0)
    got, _ = _run_check(fuser, gt, given)
    assert all(got[k] == 0 for k in E.COUNTS)
    assert all(math.isnan(got[k]) for k in E.KEYS)


@pytest.mark.parametrize("gshape", [None, (50, 90), (23, 41)])
def test_odd_sizes(fuser, gshape):
    """67 x 35: no multiple of the wave or of the tile; gt of the same size (both tiles staged),
    larger and smaller in non-integer ratios (gathered)."""
    gh, gw = gshape or (None, None)
    gt, given = _maps(35, 67, gh, gw, seed=4)
    got, _ = _run_check(fuser, gt, given)
    assert got["n_lap5"] > 0


@pytest.mark.parametrize("gshape", [None, (75, 300)])
def test_multiple_blocks(fuser, gshape):
    """2 * tile + 3 in x and in y: three blocks each way, the last one 3 pixels wide / tall."""
    w, h = 2 * TILE_X + 3, 2 * TILE_Y + 3
    gh, gw = gshape or (None, None)
    gt, given = _maps(h, w, gh, gw, seed=5)
    _run_check(fuser, gt, given)


def test_batch_equals_single(fuser):
    """Batch 3, different content: each panorama's struct and maps equal its own batch-1 call
    bit for bit."""
    h, w = 35, 2 * TILE_X + 3
    pairs = [_maps(h, w, seed=10 + b, zeros=0.02 * (b + 1)) for b in range(3)]
    gt = _dev(np.stack([p[0] for p in pairs]))
    given = _dev(np.stack([p[1] for p in pairs]))
    out = torch.zeros((3, 8), dtype=torch.int64, device=DEV)
    planes = [torch.empty((3, h, w), dtype=torch.float64, device=DEV) for _ in range(3)]
    fuser.edge_metrics_async(gt, given, out, *planes)
    fuser.synchronize()
    for b in range(3):
        o1 = torch.zeros((1, 8), dtype=torch.int64, device=DEV)
        p1 = [torch.empty((1, h, w), dtype=torch.float64, device=DEV) for _ in range(3)]
        fuser.edge_metrics_async(gt[b:b + 1].contiguous(), given[b:b + 1].contiguous(), o1, *p1)
        fuser.synchronize()
        assert torch.equal(out[b], o1[0]), b
        for k in range(3):
            assert torch.equal(planes[k][b].view(torch.int64), p1[k][0].view(torch.int64)), (b, k)
    assert len({tuple(out[b].tolist()) for b in range(3)}) == 3


def test_channels(fuser):
    """gc = 3 and given_c = 3: only channel 0 counts, whatever channels 1-2 hold."""
    gt, given = _maps(35, 67, 50, 90, seed=6)
    rng = np.random.default_rng(7)
    gt3 = np.stack([gt, rng.normal(0, 1e30, gt.shape).astype(np.float32),
                    np.zeros_like(gt)], axis=-1)
    given3 = np.stack([given, np.full_like(given, np.nan),
                       rng.normal(0, 1e30, given.shape).astype(np.float32)], axis=-1)
    _run_check(fuser, gt3, given3, gt_ch0=gt, given_ch0=given)
    gt, given = _maps(35, 67, seed=8)  # the staged path with channels
    gt3 = np.stack([gt, np.full_like(gt, -5.0), np.full_like(gt, 1e30)], axis=-1)
    given3 = np.stack([given, np.full_like(given, np.nan), np.zeros_like(given)], axis=-1)
    _run_check(fuser, gt3, given3, gt_ch0=gt, given_ch0=given)


def test_float_given_out_of_range(fuser):
    """The given map has no validity test: negative and > 1 values count like any other."""
    gt, _ = _maps(35, 67, seed=9)
    given = np.random.default_rng(9).uniform(-2.0, 3.0, (35, 67)).astype(np.float32)
    assert (given < 0).any() and (given > 1).any()
    _run_check(fuser, gt, given)


@pytest.mark.parametrize("gshape", [None, (50, 90)])
def test_u16_given(fuser, gshape):
    gh, gw = gshape or (None, None)
    gt, _ = _maps(35, 67, gh, gw, seed=11)
    given16 = np.random.default_rng(11).integers(0, 65536, (35, 67)).astype(np.uint16)
    given16[0, 0], given16[1, 1] = 0, 65535
    _run_check(fuser, gt, given16)


def test_sobel_list_as_written(fuser):
    """Isolated zero gt pixels: the Sobel count follows the reference's list (Depth.cpp:2747-2748
    never tests val[1][0] and val[2][0]), not a nine-tap test."""
    gt, given = _maps(35, 67, seed=12, zeros=0.0)
    gt[5::6, 4::7] = 0.0
    got, ref = _run_check(fuser, gt, given)
    strict = E.edge_metrics(gt, given, strict_sobel=True)
    assert got["n_sobel"] == ref["n_sobel"]
    assert got["n_sobel"] != strict["n_sobel"]
    assert got["n_sobel"] > strict["n_sobel"] > 0


@pytest.mark.parametrize("gshape", [None, (50, 90)])
def test_validity_threshold(fuser, gshape):
    """gt taps on both sides of the threshold: (double)tap < 1e-4 separates the two floats that
    neighbour 1e-4 (the kernel decides it in fp32)."""
    below, above = np.float32(float.fromhex("0x1.a36e2ep-14")), np.float32(float.fromhex("0x1.a36e30p-14"))
    assert float(below) < 1e-4 <= float(above) and np.nextafter(below, np.float32(1)) == above
    rng = np.random.default_rng(16)
    shape = gshape or (35, 67)
    gt = rng.choice(np.array([below, above, 0.5, 0.25], np.float32), size=shape,
                    p=[0.04, 0.32, 0.32, 0.32]).astype(np.float32)
    _, given = _maps(35, 67, seed=16)
    got, _ = _run_check(fuser, gt, given)
    assert 0 < got["n_lap5"] < got["n_sobel"] < 33 * 65


@pytest.mark.parametrize("gshape", [None, (50, 90)])
def test_all_zero_gt(fuser, gshape):
    _, given = _maps(35, 67, seed=13)
    gt = np.zeros(gshape or (35, 67), np.float32)
    got, _ = _run_check(fuser, gt, given)
    assert all(got[k] == 0 for k in E.COUNTS)
    assert all(math.isnan(got[k]) for k in E.KEYS)


def test_deterministic(fuser):
    h, w = 2 * TILE_Y + 3, 2 * TILE_X + 3
    gt, given = _maps(h, w, seed=14)
    gt, given = _dev(gt[None]), _dev(given[None])
    outs = []
    for _ in range(2):
        o = torch.zeros((1, 8), dtype=torch.int64, device=DEV)
        fuser.edge_metrics_async(gt, given, o)
        fuser.synchronize()
        outs.append(o.cpu())
    assert torch.equal(outs[0], outs[1])
    assert outs[0][0, 5] > 0


@pytest.fixture(scope="module")
def merged(fuser):
    """C2 results of two synthetic panoramas (fused on the GPU) and their ground truth, as
    tests/test_gpu_metrics.py builds them."""
    nb = 2
    lay = PL.config_layout("C2")
    fuser.set_tiles(lay)
    seeds = pf_synth.seeds_for(nb, 20261015 + 977)
    emap = pf_synth.baseline_emap(seeds, 512, 256)
    gt = pf_synth.scene_depth(seeds, 2048, 1024)
    tiles, total = O.make_tiles(lay)
    resp = pf_synth.responses(seeds, lay.ntiles)
    data = np.stack([O.warp_depth(gt[b].numpy(), tiles, total,
                                  O.responses(resp[b * lay.ntiles:(b + 1) * lay.ntiles]))
                     for b in range(nb)])
    out = torch.zeros((nb, 1024, 2048), dtype=torch.int16, device=DEV)
    fuser.merge(emap.to(DEV).contiguous(), _dev(data.reshape(nb, -1)), out, PL.ZENITH_RANGE)
    torch.cuda.synchronize()
    return gt.numpy(), out


def test_workload_shape(fuser, merged):
    """The flagship shape: 2048 x 1024 u16 results against their gt, batch 2 (gt of the result's
    size: both tiles staged in LDS)."""
    gt, out = merged
    gt = gt.copy()
    gt[:, 100:140, 300:900] = 0.0  # a black band, so the validity tests have work
    res, gl, vl, ae = fuser.edge_metrics(_dev(gt), out, maps=True)
    res16 = out.cpu().numpy().view(np.uint16)
    for b in range(2):
        ref, rmaps = E.edge_metrics(gt[b], E.u16_to_float(res16[b]), maps=True)
        _check(res[b], ref, 2048, 1024)
        assert 0 < ref["n_lap5"] < ref["n_sobel"] < 2046 * 1022
        for name, t in (("gt_lap", gl), ("given_lap", vl), ("lap_ae", ae)):
            assert np.array_equal(t[b].cpu().numpy(), rmaps[name]), (b, name)


def test_bad_arguments(fuser):
    L, h = fuser.L, fuser.h
    gt, given = _maps(8, 8, seed=15)
    gt, given = _dev(gt[None]), _dev(given[None])
    g16 = torch.zeros((1, 8, 8), dtype=torch.int16, device=DEV)
    out = torch.zeros((1, 8), dtype=torch.int64, device=DEV)
    P = panofuse._ptr

    def call(gf, gu, w=8, hh=8, batch=1):
        return L.pf_error_laplacian(h, P(gt), 8, 8, 1, gf, gu, w, hh, 1, batch, P(out),
                                    None, None, None)
    assert call(P(given), P(g16)) == panofuse.PF_EINVAL
    assert b"exactly one" in L.pf_last_error(h)
    assert call(None, None) == panofuse.PF_EINVAL
    assert call(P(given), None, w=0) == panofuse.PF_EINVAL
    assert call(P(given), None, batch=0) == panofuse.PF_EINVAL
    assert call(P(given), None) == panofuse.PF_OK
    fuser.synchronize()
    with pytest.raises(panofuse.PanofuseError):
        fuser.edge_metrics_async(gt, given, None)
