"""The direct tile stitch (pf_stitch), the Laplacian self-check (pf_laplacian_residual) and the
fusion with the check at every level (pf_fuse_check) on the GPU, bit for bit against the CPU
restatement tests/stitch_ref.py -- which tests/test_stitch_ref.py pins to the compiled reference
(tests/golden/stitch_ref.npz).

Stitch cases: the C1 layout with 256^2 tiles at 512x256, 100x50 and 101x51, batch 1 and 3, with
and without coefficients; 101x51 has an odd pixel count, so panorama 1 of a batch starts on an odd
u16 offset, and a second call writes into a buffer shifted by one u16 so that panoramas 0 and 2
do (the kernel stores dword pairs cut relative to each plane's address).  LeReS' 15 windows with
128x124 tiles at 512x256.  Constant tiles (p + 1) / 32: every pixel in two boxes holds the lower
tile's value, which tells the stitch from the smoothing map (last tile wins).  The golden's inputs
reproduce the golden.

Residual cases: the 8x8 hand cases of test_stitch_ref, a random 130x70 plane (rows 5..64: 7,424
terms, more than one 1024-pixel chunk) in a batch of 3 with markers scattered in the targets, and
PF_EINVAL for a band without interior.  The kernel is the plain one-wave chain, so there is no
redo path to force.

pf_fuse_check at C1 (512x256) and at 500x248 (tests/test_fuse_shapes.py: level 0 takes the
per-sweep form, the others the streamed one): its u16 equals pf_fuse's, every err[l] equals the
restatement on the planes pf_fuse_targets / pf_fuse_level return, and is finite and >= 0.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import panofuse  # noqa: E402
import pf_layouts as PL  # noqa: E402
import pf_synth  # noqa: E402
import pyoracle as O  # noqa: E402
import stitch_ref as S  # noqa: E402
from test_stitch_ref import GOLDEN, _harmonic_plane  # noqa: E402

ZR = PL.ZENITH_RANGE
DEV = "cuda:0"
f32 = np.float32


@pytest.fixture(scope="module")
def fuser():
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected on a host without a GPU")
    return panofuse.Fuser(0)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _scene_tiles(lay, n, base):
    tiles, total = O.make_tiles(lay)
    seeds = pf_synth.seeds_for(n, base)
    gt = pf_synth.scene_depth(seeds, 512, 256).numpy()
    resp = pf_synth.responses(seeds, lay.ntiles)
    nt = lay.ntiles
    data = np.stack([O.warp_depth(gt[b], tiles, total, O.responses(resp[b * nt:(b + 1) * nt]))
                     for b in range(n)])
    return tiles, data


def _coeffs(n, ntiles, seed):
    rng = np.random.default_rng(seed)
    c = np.zeros((n, ntiles, 4), np.float32)
    c[:, :, 0] = rng.uniform(-0.3, 0.3, (n, ntiles))
    c[:, :, 1] = rng.uniform(-0.3, 0.3, (n, ntiles))
    c[:, :, 2] = rng.uniform(0.8, 1.2, (n, ntiles))
    c[:, :, 3] = rng.uniform(-0.05, 0.05, (n, ntiles))
    return c


@pytest.fixture(scope="module")
def c1():
    lay = PL.config_layout("C1")
    tiles, data = _scene_tiles(lay, 3, 20261020)
    return lay, tiles, data, _coeffs(3, lay.ntiles, 7)


def _stitch(fuser, data, W, H, coeffs=None, shift=0):
    B = data.shape[0]
    flat = torch.full((B * W * H + shift + 1,), -1, dtype=torch.int16, device=DEV)
    out = flat[shift:shift + B * W * H].view(B, H, W)
    fuser.stitch(_dev(data), out, coeffs=None if coeffs is None else _dev(coeffs))
    torch.cuda.synchronize()
    host = flat.cpu().numpy().view(np.uint16)
    assert (host[:shift] == 0xFFFF).all() and host[-1] == 0xFFFF  # nothing outside the planes
    return host[shift:shift + B * W * H].reshape(B, H, W)


@pytest.fixture(scope="module")
def c1_ref(c1):
    """The restatement of every C1 case, computed once: {(W, H, with coeffs): [3][H][W]}."""
    lay, tiles, data, coeffs = c1
    ref = {}
    for (W, H) in [(512, 256), (100, 50), (101, 51)]:
        for wc in (False, True):
            ref[(W, H, wc)] = np.stack([S.stitch(tiles, data[b], W, H, coeffs[b] if wc else None)
                                        for b in range(3)])
    return ref


@pytest.mark.parametrize("with_coeffs", [False, True], ids=["plain", "coeffs"])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("W,H", [(512, 256), (100, 50), (101, 51)])
def test_stitch_equals_restatement(fuser, c1, c1_ref, W, H, batch, with_coeffs):
    lay, tiles, data, coeffs = c1
    fuser.set_tiles(lay)
    ref = c1_ref[(W, H, with_coeffs)][:batch]
    for shift in (0, 1):  # shift 1: the buffer itself starts on an odd u16 offset
        got = _stitch(fuser, data[:batch], W, H, coeffs[:batch] if with_coeffs else None, shift)
        bad = int((got != ref).sum())
        print(f"{W}x{H} batch {batch} coeffs {with_coeffs} shift {shift}: {bad} pixels differ")
        assert bad == 0
    assert int((ref != 0).sum()) > W  # non-trivial output


def test_stitch_leres_windows(fuser):
    lay = PL.leres_layout(tile_w=128, tile_h=124)
    tiles, data = _scene_tiles(lay, 1, 20261021)
    fuser.set_tiles(lay)
    stats = {}
    ref = S.stitch(tiles, data[0], 512, 256, stats=stats)
    got = _stitch(fuser, data, 512, 256)[0]
    print(f"LeReS 512x256: outside its tile {stats['outside']}, differing {int((got != ref).sum())}")
    assert np.array_equal(got, ref)


def test_stitch_first_tile_wins(fuser, c1):
    lay, tiles, _, _ = c1
    fuser.set_tiles(lay)
    data = np.concatenate([np.full(256 * 256, (p + 1) / 32.0, np.float32)
                           for p in range(lay.ntiles)])[None]
    W, H = 512, 256
    got = _stitch(fuser, data, W, H)[0]
    cnt, first = S.cover(tiles, W, H)
    want = S.quantize((first + 1).astype(np.float32) / f32(32.0))
    want[first < 0] = 0
    twice = cnt > 1
    assert int(twice.sum()) > 500
    assert np.array_equal(got[twice], want[twice])  # the lower tile's value
    assert np.array_equal(got, want)
    # the smoothing map's choice (the last covering tile) differs on those pixels
    bx = S.boxes(tiles, W, H)
    ys, xs = np.nonzero(twice)
    last = [max(p for p, (x0, x1, y0, y1) in enumerate(bx)
                if min(x0, x1) <= x <= max(x0, x1) and y0 <= y <= y1) for y, x in zip(ys, xs)]
    assert (np.array(last) != first[twice]).all()


@pytest.mark.parametrize("W,H", [(100, 50), (101, 51)])
def test_stitch_reproduces_the_golden(fuser, W, H):
    g = np.load(GOLDEN)
    fuser.set_tiles(S.golden_layout())
    data = S.golden_tiles(g["tiles_u8"]).reshape(1, -1)
    got = _stitch(fuser, data, W, H, g["abcd"][None])[0]
    assert np.array_equal(got, g[f"out_{W}x{H}"])


def test_stitch_map_follows_the_layout(fuser, c1):
    """The cached map is per layout: another layout at the same size, then the first one again."""
    lay, tiles, data, _ = c1
    fuser.set_tiles(lay)
    a = _stitch(fuser, data[:1], 100, 50)[0]
    g = np.load(GOLDEN)
    fuser.set_tiles(S.golden_layout())
    b = _stitch(fuser, S.golden_tiles(g["tiles_u8"]).reshape(1, -1), 100, 50, g["abcd"][None])[0]
    assert np.array_equal(b, g["out_100x50"])
    fuser.set_tiles(lay)
    assert np.array_equal(_stitch(fuser, data[:1], 100, 50)[0], a)


# ---------------------------------------------------------------------------------------------
def _residual(fuser, buf, ln, h0, h1):
    err = fuser.laplacian_residual(_dev(buf), _dev(ln), h0, h1)
    torch.cuda.synchronize()
    return err.cpu().numpy()


def test_residual_hand_cases(fuser):
    buf, ln = _harmonic_plane()
    planes, targets = [buf.copy()], [ln.copy()]
    b1 = buf.copy()
    b1[3, 4] += f32(0.125)
    planes.append(b1)
    targets.append(ln.copy())
    l2 = ln.copy()
    l2.view(np.uint32)[4, 2] = S.NAN_MARKER
    planes.append(buf.copy())
    targets.append(l2)
    got = _residual(fuser, np.stack(planes), np.stack(targets), 1, 6)
    want = np.array([S.laplacian_residual(p, t, 1, 6) for p, t in zip(planes, targets)], f32)
    print("hand cases:", got, want)
    assert got[0] == 0.0 and got[1] == f32(0.125 ** 2 * 1.25)
    assert got[2] == S.sq_step(f32(0), ln[4, 2]) and got[2] > 0
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_residual_random_planes_with_markers(fuser):
    rng = np.random.default_rng(11)
    B, h, w, h0, h1 = 3, 70, 130, 5, 64
    buf = rng.random((B, h, w)).astype(np.float32)
    ln = (rng.standard_normal((B, h, w)) * 0.1).astype(np.float32)
    mark = rng.random((B, h, w)) < 0.05
    ln.view(np.uint32)[mark] = S.NAN_MARKER
    got = _residual(fuser, buf, ln, h0, h1)
    want = np.array([S.laplacian_residual(buf[b], ln[b], h0, h1) for b in range(B)], f32)
    print("random planes:", got, want, "terms", (h1 - h0 - 1) * (w - 2))
    assert (h1 - h0 - 1) * (w - 2) > 1024 and int(mark[:, h0 + 1:h1, 1:-1].sum()) > 100
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.isfinite(got).all() and (got > 0).all()


def test_residual_rejects_a_band_without_interior(fuser):
    z = torch.zeros((1, 8, 8), dtype=torch.float32, device=DEV)
    for h0, h1, in [(3, 4), (-1, 6), (1, 8)]:
        with pytest.raises(panofuse.PanofuseError) as e:
            fuser.laplacian_residual(z, z, h0, h1)
        assert e.value.code == panofuse.PF_EINVAL
    z2 = torch.zeros((1, 8, 2), dtype=torch.float32, device=DEV)
    with pytest.raises(panofuse.PanofuseError) as e:
        fuser.laplacian_residual(z2, z2, 1, 6)
    assert e.value.code == panofuse.PF_EINVAL


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,eshape", [(512, 256, (128, 64)), (500, 248, (77, 31))])
def test_fuse_check(fuser, c1, W, H, eshape):
    lay, tiles, data, coeffs = c1
    fuser.set_tiles(lay)
    ew, eh = eshape
    emap = _dev(pf_synth.baseline_emap(pf_synth.seeds_for(1, 20261022), ew, eh).numpy()
                .astype(np.float32))
    t, k = _dev(data[:1]), _dev(coeffs[:1])
    ref = torch.zeros((1, H, W), dtype=torch.int16, device=DEV)
    fuser.fuse(emap, t, ref, ZR, coeffs=k)
    out = torch.zeros((1, H, W), dtype=torch.int16, device=DEV)
    err = fuser.fuse_check(emap, t, ZR, W, out_h=H, coeffs=k, out=out)
    fuser.synchronize()
    assert torch.equal(out, ref)
    err = err.cpu().numpy()
    nlev = panofuse.level_info(W, H, ZR, 0)[5]
    assert err.shape == (nlev,) and np.isfinite(err).all() and (err >= 0).all()
    prev, want = None, []
    for l in range(nlev):
        w, h, h0, h1 = panofuse.level_info(W, H, ZR, l)[:4]
        ln = torch.zeros((h, w), dtype=torch.float32, device=DEV)
        buf = torch.zeros((h, w), dtype=torch.float32, device=DEV)
        fuser.fuse_targets(t, k, W, ZR, l, ln, out_h=H)
        fuser.fuse_level(emap, prev, ln, None, W, ZR, l, buf, out_h=H)
        fuser.synchronize()
        want.append(S.laplacian_residual(buf.cpu().numpy(), ln.cpu().numpy(), h0, h1))
        prev = buf
    want = np.array(want, f32)
    print(f"fuse_check {W}x{H}: err {err} restatement {want}")
    assert np.array_equal(err.view(np.uint32), want.view(np.uint32))
    # without out: the same numbers
    err2 = fuser.fuse_check(emap, t, ZR, W, out_h=H, coeffs=k)
    fuser.synchronize()
    assert np.array_equal(err2.cpu().numpy().view(np.uint32), err.view(np.uint32))
