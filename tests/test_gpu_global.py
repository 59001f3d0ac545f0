"""GPU global result-to-baseline registration, u16 transform, MedianScaling and
CopyInvalidPixels (csrc/pf_global.hip) against the CPU restatement (tests/global_ref.py) and the
compiled reference's recorded results (tests/golden/global_ref.npz).

Fit shapes: 512x256 over 128x64 (94,720 samples: five full chunks of 16,384 and a ragged sixth),
100x50 over 64x33 (odd sizes, both clamps fire) and 64x32 over 16x8 (one partial chunk).
"""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import global_ref as G  # noqa: E402
import panofuse  # noqa: E402
import pf_layouts as PL  # noqa: E402
import pf_synth  # noqa: E402
import pyoracle as O  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "global_ref.npz")
ZR = PL.ZENITH_RANGE
DEV = "cuda:0"
NMAP = 5


@pytest.fixture(scope="module")
def fuser():
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected on a host without a GPU")
    return panofuse.Fuser(0)


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    assert tuple(z["zenith_range"]) == tuple(np.float32(v) for v in ZR)
    return z


@pytest.fixture(scope="module")
def fits(golden):
    """Golden fit cases 3, 1, 0 with the restatement's fit of each (read-only)."""
    out = {}
    for k in (3, 1, 0):
        emap, data = golden[f"fit_emap{k}"], golden[f"fit_data{k}"]
        c64, abcd, s = G.register_global(emap, data, ZR)
        out[k] = {"emap": emap, "data": data, "c64": c64, "abcd": abcd,
                  "summary": G.summary_row(s), "golden": golden["fit_abcd"][k]}
    return out


@pytest.fixture(scope="module")
def trio(fits):
    """Three distinct 512x256 panoramas over distinct 128x64 baselines."""
    emap, data = fits[3]["emap"], fits[3]["data"]
    emaps = [emap, (emap[:, ::-1] * np.float32(0.9)).astype(np.float32),
             np.roll(emap, 17, axis=1)]
    datas = [data, np.ascontiguousarray(data[:, ::-1]),
             (np.roll(data, 40, axis=1) // 2 + 9000).astype(np.uint16)]
    return [np.ascontiguousarray(e) for e in emaps], [np.ascontiguousarray(d) for d in datas]


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).to(DEV)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _register(fuser, emaps, datas, apply=False):
    """register_global on a batch: (coeffs f32, coeffs64, summary, data afterwards as u16)."""
    B = len(emaps)
    t_emap, t_data = _dev(np.stack(emaps)), _dev(np.stack(datas))
    cf = torch.zeros((B, 4), dtype=torch.float32, device=DEV)
    c64 = torch.zeros((B, 4), dtype=torch.float64, device=DEV)
    sm = torch.zeros((B, 4), dtype=torch.float64, device=DEV)
    fuser.register_global(t_emap, t_data, ZR, apply=apply, coeffs=cf, coeffs64=c64, summary=sm)
    fuser.synchronize()
    return (cf.cpu().numpy(), c64.cpu().numpy(), sm.cpu().numpy(),
            t_data.cpu().numpy().view(np.uint16))


@pytest.mark.parametrize("k", [3, 1, 0])
def test_fit_bit_exact(fuser, fits, k):
    f = fits[k]
    cf, c64, sm, after = _register(fuser, [f["emap"]], [f["data"]])
    print(f"case {k}: gpu {c64[0]} ref {f['c64']} summary {sm[0]} ref {f['summary']}")
    assert np.array_equal(after[0], f["data"])  # apply = 0 leaves the result alone
    assert np.array_equal(_bits(c64[0]), _bits(f["c64"]))
    assert np.array_equal(_bits(sm[0]), _bits(f["summary"]))
    assert np.array_equal(_bits(cf[0]), _bits(f["golden"]))  # the compiled reference's abcd
    assert sm[0, 1] < sm[0, 0]


def test_batch_equals_single_calls(fuser, trio):
    emaps, datas = trio
    cf, c64, sm, _ = _register(fuser, emaps, datas)
    assert len({c64[b].tobytes() for b in range(3)}) == 3  # distinct panoramas, distinct fits
    for b in range(3):
        cf1, c641, sm1, _ = _register(fuser, [emaps[b]], [datas[b]])
        assert np.array_equal(_bits(c64[b]), _bits(c641[0])), b
        assert np.array_equal(_bits(cf[b]), _bits(cf1[0])), b
        assert np.array_equal(_bits(sm[b]), _bits(sm1[0])), b


@pytest.mark.parametrize("k", [3, 1, 0])
def test_apply_equals_the_restatement(fuser, fits, k):
    f = fits[k]
    cf, _, _, after = _register(fuser, [f["emap"]], [f["data"]], apply=True)
    assert np.array_equal(_bits(cf[0]), _bits(f["abcd"]))
    want = G.result_transform(f["data"], ZR, f["abcd"])
    h0, h1 = G.band(f["data"].shape[0], ZR)
    assert np.array_equal(after[0], want)
    assert np.array_equal(after[0][:h0], f["data"][:h0])
    assert np.array_equal(after[0][h1 + 1:], f["data"][h1 + 1:])
    assert not np.array_equal(after[0][h0:h1 + 1], f["data"][h0:h1 + 1])


def test_result_transform_batch_and_edge_coefficients(fuser, trio):
    """pf_result_transform alone on a batch with per-panorama coefficients, NaN among them, on a
    band that starts at an odd element offset (the unaligned path)."""
    _, datas = trio
    coeffs = np.array([[0.5, -0.25, 0.9, 0.01], [np.nan, 0, 0, 0], [0, 0, 0, 5]], np.float32)
    t = _dev(np.stack(datas))
    fuser.result_transform(t, ZR, _dev(coeffs))
    fuser.synchronize()
    got = t.cpu().numpy().view(np.uint16)
    for b in range(3):
        assert np.array_equal(got[b], G.result_transform(datas[b], ZR, coeffs[b])), b
    odd = np.ascontiguousarray(datas[0][:51, :99])  # 99 wide: rows start at odd offsets
    t = _dev(odd[None])
    fuser.result_transform(t, ZR, _dev(coeffs[:1]))
    fuser.synchronize()
    assert np.array_equal(t.cpu().numpy().view(np.uint16)[0],
                          G.result_transform(odd, ZR, coeffs[0]))


def test_end_to_end_c1_merge_then_global_fit(fuser):
    """The C1 merge of the synthetic inputs, then the global fit and transform: the oracle's merge
    passed through the restatement."""
    lay = PL.config_layout("C1")
    seeds = pf_synth.seeds_for(1)
    emap = pf_synth.baseline_emap(seeds, 128, 64)
    gt = pf_synth.scene_depth(seeds, 512, 256)
    tiles_o, total = O.make_tiles(lay)
    resp = pf_synth.responses(seeds, lay.ntiles)
    tile_data = O.warp_depth(gt[0].numpy(), tiles_o, total, O.responses(resp))
    ref_out, _ = O.merge(emap[0].numpy(), tiles_o, tile_data.copy(), 512, ZR)
    c64, abcd, s = G.register_global(emap[0].numpy(), ref_out, ZR)
    want = G.result_transform(ref_out, ZR, abcd)

    fuser.set_tiles(lay)
    t_emap = emap.to(DEV).contiguous()
    t_tiles = torch.from_numpy(tile_data).to(DEV).reshape(1, -1).contiguous()
    out = torch.zeros((1, 256, 512), dtype=torch.int16, device=DEV)
    fuser.merge(t_emap, t_tiles, out, ZR)
    sm = torch.zeros((1, 4), dtype=torch.float64, device=DEV)
    d64 = torch.zeros((1, 4), dtype=torch.float64, device=DEV)
    fuser.register_global(t_emap, out, ZR, apply=True, coeffs64=d64, summary=sm)
    fuser.synchronize()
    got = out.cpu().numpy().view(np.uint16)[0]
    sm = sm.cpu().numpy()[0]
    print(f"abcd {abcd} cost {sm[0]} -> {sm[1]} ({int(sm[2])} iterations)")
    assert np.array_equal(_bits(d64.cpu().numpy()[0]), _bits(c64))
    assert np.array_equal(got, want)
    assert sm[1] < sm[0]


def test_bad_sizes_are_refused(fuser, fits):
    f = fits[0]
    t_emap, t_data = _dev(f["emap"][None]), _dev(f["data"][None])
    with pytest.raises(panofuse.PanofuseError) as e:
        fuser.register_global(t_emap, t_data, (0.5, 3.2))  # rows past the last one
    assert e.value.code == panofuse.PF_EINVAL and "rows" in str(e.value)
    with pytest.raises(panofuse.PanofuseError):
        fuser.result_transform(t_data, (2.0, 1.0), _dev(np.zeros((1, 4), np.float32)))
    with pytest.raises(panofuse.PanofuseError):
        fuser.median_scale(t_emap[:, :, :0], t_emap)


def _median(fuser, m0s, m1s):
    t0, t1 = _dev(np.stack(m0s)), _dev(np.stack(m1s))
    med = torch.full((len(m0s), 2), -1.0, dtype=torch.float32, device=DEV)
    st = torch.full((len(m0s),), -1, dtype=torch.int32, device=DEV)
    fuser.median_scale(t0, t1, medians=med, status=st)
    fuser.synchronize()
    return t0.cpu().numpy(), med.cpu().numpy(), st.cpu().numpy(), t1.cpu().numpy()


@pytest.mark.parametrize("k", range(NMAP))
def test_median_scale_equals_the_compiled_reference(fuser, golden, k):
    m0, m1 = golden[f"map0_{k}"], golden[f"map1_{k}"]
    scaled, med, st, m1_after = _median(fuser, [m0], [m1])
    ret, ra, rb = golden["med"][k]
    assert ret == 1 and st[0] == 0
    assert np.array_equal(_bits(med[0]), _bits(np.array([ra, rb], np.float32)))
    assert np.array_equal(_bits(scaled[0]), golden[f"scaled{k}"])
    assert np.array_equal(_bits(m1_after[0]), _bits(m1))


def test_median_scale_batch_with_a_dead_map(fuser, golden):
    m0, m1 = golden["map0_1"], golden["map1_1"]
    dead = np.zeros_like(m0)
    dead[3, 5], dead[4, 6], dead[5, 7] = 1.0, np.nan, 5e-5
    scaled, med, st, _ = _median(fuser, [dead, m0], [m1, m1])
    assert st.tolist() == [1, 0]
    assert np.array_equal(_bits(scaled[0]), _bits(dead))
    assert med[0].tolist() == [0.0, 0.0]
    assert np.array_equal(_bits(scaled[1]), golden["scaled1"])
    # the other way round: map 1 without a valid pixel
    scaled, med, st, _ = _median(fuser, [m0, m0], [m1, dead])
    assert st.tolist() == [0, 1]
    assert np.array_equal(_bits(scaled[0]), golden["scaled1"])
    assert np.array_equal(_bits(scaled[1]), _bits(m0))


def test_median_scale_nan_is_invalid(fuser, golden):
    m0 = golden["map0_0"].copy()
    m1 = golden["map1_0"]
    m0[::5, ::7] = np.nan
    ok, a, b, want = G.median_scale(m0, m1)
    scaled, med, st, _ = _median(fuser, [m0], [m1])
    assert ok and st[0] == 0
    assert np.array_equal(_bits(med[0]), _bits(np.array([a, b], np.float32)))
    assert np.array_equal(_bits(scaled[0]), _bits(want))


@pytest.mark.parametrize("k", range(NMAP))
def test_copy_invalid_equals_the_compiled_reference(fuser, golden, k):
    m0, m1 = golden[f"map0_{k}"], golden[f"map1_{k}"]
    nan_ref = m1.copy()
    nan_ref.reshape(-1)[::11] = np.nan  # a NaN reference pixel is not copied
    t = _dev(np.stack([m0, m0]))
    fuser.copy_invalid(t, _dev(np.stack([m1, nan_ref])))
    fuser.synchronize()
    got = t.cpu().numpy()
    assert np.array_equal(_bits(got[0]), golden[f"masked{k}"])
    assert np.array_equal(_bits(got[1]), _bits(G.copy_invalid(m0, nan_ref)))
