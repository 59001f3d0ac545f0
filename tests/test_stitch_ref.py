"""CPU checks of the stitch / Laplacian-check restatement (tests/stitch_ref.py), which the GPU
tests (tests/test_gpu_stitch.py) hold csrc/pf_stitch.hip to bit for bit.

* On tests/golden/stitch_ref.npz (tools/make_stitch_golden.py: the reference's own SetWindow,
  Depth2DepthTransform, SphericalTo2D and Value under the restated loop of Depth.cpp:822-857,
  C1 windows with 64 x 64 tiles) the restatement's u16 plane equals the compiled reference's bit
  for bit at 100 x 50 and 101 x 51, no index leaves its tile, and the pixels that lie in more
  than one box (170 and 173, the harness's own counts) hold the first tile's value.
* The residual restatement gives 0 on a plane whose Laplacian equals its targets, the
  hand-computed five-term value after one interior pixel is perturbed, and counts a pixel that
  carries the un-windowed marker with target 0.
"""
import os

import numpy as np
import pytest

import pyoracle as O
import stitch_ref as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stitch_ref.npz")
SIZES = [(100, 50), (101, 51)]
f32 = np.float32


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def golden_tiles():
    return O.make_tiles(S.golden_layout())[0]


@pytest.mark.parametrize("W,H", SIZES)
def test_stitch_equals_the_compiled_reference(golden, golden_tiles, W, H):
    data = S.golden_tiles(golden["tiles_u8"]).ravel()
    stats = {}
    got = S.stitch(golden_tiles, data, W, H, golden["abcd"], stats)
    ref = golden[f"out_{W}x{H}"]
    cnt, first = S.cover(golden_tiles, W, H)
    covered, twice = [int(v) for v in golden[f"counts_{W}x{H}"]]
    print(f"{W}x{H}: covered {int((cnt > 0).sum())} in two boxes {int((cnt > 1).sum())} outside "
          f"{stats['outside']} differing {int((got != ref).sum())}")
    assert stats["outside"] == 0
    assert (int((cnt > 0).sum()), int((cnt > 1).sum())) == (covered, twice)
    assert twice > 100  # first-tile-wins is exercised
    assert np.array_equal(got, ref)
    assert not ref[cnt == 0].any() and ref[cnt > 0].any()


def test_first_tile_wins_where_boxes_overlap(golden_tiles):
    """Tile p constant at (p + 1) / 32: a pixel in two boxes holds the lower tile's value -- the
    smoothing map (last tile wins, x1 exclusive) would not."""
    W, H = 100, 50
    n = len(golden_tiles)
    data = np.concatenate([np.full(S.GOLDEN_TILE ** 2, (p + 1) / 32.0, np.float32)
                           for p in range(n)])
    got = S.stitch(golden_tiles, data, W, H)
    cnt, first = S.cover(golden_tiles, W, H)
    want = S.quantize(((first + 1).astype(np.float32) / f32(32.0)))
    want[first < 0] = 0
    assert np.array_equal(got, want)
    bx = S.boxes(golden_tiles, W, H)
    for y, x in zip(*np.nonzero(cnt > 1)):
        inside = [p for p, (x0, x1, y0, y1) in enumerate(bx)
                  if min(x0, x1) <= x <= max(x0, x1) and y0 <= y <= y1]
        assert len(inside) >= 2 and first[y, x] == inside[0]
        assert got[y, x] == S.quantize(f32((inside[0] + 1) / 32.0))


def _harmonic_plane():
    """An 8 x 8 plane and targets with Laplacian == target exactly: values k / 64 keep every sum
    exact in fp32, and the targets are computed with the same expression."""
    rng = np.random.default_rng(3)
    buf = (rng.integers(0, 64, (8, 8)) / 64.0).astype(np.float32)
    ln = np.zeros((8, 8), np.float32)
    s = ((buf[1:-1, :-2] + buf[1:-1, 2:]) + buf[:-2, 1:-1]) + buf[2:, 1:-1]
    ln[1:-1, 1:-1] = buf[1:-1, 1:-1] - s / f32(4)
    return buf, ln


def test_residual_zero_when_laplacian_equals_targets():
    buf, ln = _harmonic_plane()
    assert S.laplacian_residual(buf, ln, 1, 6) == 0.0


def test_residual_of_one_perturbed_pixel_is_five_terms():
    buf, ln = _harmonic_plane()
    e = f32(0.125)  # exact in every sum
    buf[3, 4] += e  # interior of rows 2..5, columns 1..6
    # the pixel's own Laplacian moves by e, its four neighbours' by -e/4; row-major order:
    # (2,4), (3,3), (3,4), (3,5), (4,4)
    want = f32(0)
    for d in (-e / 4, -e / 4, e, -e / 4, -e / 4):
        want = S.sq_step(want, f32(d))
    got = S.laplacian_residual(buf, ln, 1, 6)
    assert got == want and got == f32(0.125 ** 2 * 1.25)


def test_residual_marker_pixel_counts_with_target_zero():
    buf, ln = _harmonic_plane()
    bits = ln.view(np.uint32)
    lap = ln[4, 2].copy()
    assert lap != 0
    bits[4, 2] = S.NAN_MARKER
    assert S.laplacian_residual(buf, ln, 1, 6) == S.sq_step(f32(0), lap)


def test_residual_rejects_a_band_without_interior():
    buf, ln = _harmonic_plane()
    with pytest.raises(ValueError):
        S.laplacian_residual(buf, ln, 3, 4)
