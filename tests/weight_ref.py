"""CPU restatement of the per-pixel tile weights (pf_register_weighted, pf_fuse_weighted,
pf_merge_weighted, pf_tile_tent_weights), composed from the oracle's building blocks and
tests/mask_ref.py's pieces.

TEST INFRASTRUCTURE ONLY.  tests/test_weight_ref.py proves the restatement: with every weight 1.0f
it is the oracle's merge bit for bit, with weights in {0, 1} it is mask_ref's masked fusion and
registration bit for bit.  tests/test_gpu_weights.py holds the library to it.

Usable weight.  u(w) = w if 0 < w < +inf in fp32, else 0.

Fusion.  Per level and tile p: the tile's data carries NaN wherever u(w) == 0 or the (transformed)
value is not finite, so O.targets_subset(tiles, p, p + 1, data_nan, lv) gives the five-point sum Lp
in std::map key order with NaN exactly where a tap does not count; the five tap elements come from
O.probe_taps on the one-tile sub-array (clamped as the gather clamps them; the centre is entry 2)
and wmin is the fp32 minimum of u(w) over them.  Tiles in ascending order: acc = acc + wmin * Lp
and ws = ws + wmin in fp32, one rounding each; the target is acc * (1 / ws), the marker where
ws == 0.  Then O.seed_level0 / O.upsample, O.jacobi, O.quantize as in pfo_solve_depth_all.

Registration.  mask_ref.reg_sums's lanes and halving tree with every term times (double)w; the
sum of w is sum 9 and the count of used samples is carried apart.  Then O.lm_moments.
"""
import numpy as np

import mask_ref as M
import pyoracle as O

f32 = np.float32
ZR = M.ZR
MARKER_BITS = np.uint32(0x7FBADBAD)  # PF_NAN_MARKER: a signalling NaN, so it is written as bits


def golden_inputs():
    """(oracle tiles, emap, tile data) of tests/golden/c1_merge.npz: the C1 layout with the stored
    u16 baseline and u8 tiles, as tests/test_oracle.py reads them."""
    import pf_layouts as PL
    from test_oracle import GOLDEN
    g = np.load(GOLDEN)
    tiles, _ = O.make_tiles(PL.config_layout("C1"))
    emap = g["emap_u16"].astype(f32) / f32(65535.0)
    data = g["tiles_u8"].astype(f32).ravel() / f32(255.0)
    return tiles, emap, data


def usable(w):
    """u(w), float32, any shape."""
    w = np.asarray(w, f32)
    with np.errstate(invalid="ignore"):
        return np.where((w > 0) & (w < np.inf), w, f32(0)).astype(f32)


def tent(tiles):
    """pf_tile_tent_weights' set for the oracle tiles: float32 [tile_elems], channel 0."""
    total = sum(t.width * t.height * t.channels for t in tiles)
    out = np.zeros(total, f32)
    for t in tiles:
        w, h, c = t.width, t.height, t.channels
        x = np.arange(w)[None, :]
        y = np.arange(h)[:, None]
        tt = np.minimum(np.minimum(x + 1, w - x), np.minimum(y + 1, h - y))
        m = (min(w, h) + 1) // 2
        val = np.minimum(tt, m).astype(f32) / f32(m)
        out[t.offset:t.offset + w * h * c:c] = val.reshape(-1)
    return out


def staged(tiles, data, weights, abcd=None):
    """The tile data as the gather stages it: a copy, transformed when abcd is given, with NaN
    at every channel-0 element whose weight is unusable or whose (transformed) value is not
    finite."""
    d = np.array(data, f32).ravel()
    if abcd is not None:
        d = M.transform(tiles, d, abcd)
    u = usable(weights).ravel()
    for t in tiles:
        sl = slice(t.offset, t.offset + t.width * t.height * t.channels, t.channels)
        v = d[sl]
        d[sl] = np.where((u[sl] > 0) & np.isfinite(v), v, f32(np.nan))
    return d


def tile_taps(tiles, p, lv):
    """(inbox bool [h][w], taps int64 [h][w][5]): the pixels of tile p's box at the level and the
    clamped element index inside the tile of each of their five taps (key order)."""
    t = tiles[p]
    one = (O.Tile * 1)()
    one[0] = t
    raw = O.probe_taps(one, lv).astype(np.int64)
    n = t.width * t.height * t.channels
    zeros = np.zeros(sum(q.width * q.height * q.channels for q in tiles), f32)
    _, c = O.targets_subset(tiles, p, p + 1, zeros, lv)
    taps = np.where(raw < 0, 0, np.where(raw >= n, n - t.channels, raw))
    return c > 0, taps


def weighted_targets(tiles, data_nan, weights, lv):
    """(Lnorm float32 [h][w] with the marker, ws float32 [h][w]) of one level."""
    u = usable(weights).ravel()
    acc = np.zeros((lv.h, lv.w), f32)
    ws = np.zeros((lv.h, lv.w), f32)
    for p in range(len(tiles)):
        s, c = O.targets_subset(tiles, p, p + 1, data_nan, lv)
        inbox, taps = tile_taps(tiles, p, lv)
        assert np.array_equal(inbox, c > 0), "every covered pixel has tap indices"
        wmin = u[tiles[p].offset + taps].min(axis=-1).astype(f32)
        ok = inbox & ~np.isnan(s)
        ok[:lv.h0 + 1] = False  # targets exist on rows h0 < Y < h1 only
        ok[lv.h1:] = False
        with np.errstate(invalid="ignore"):
            prod = (wmin * s).astype(f32)            # one fp32 multiply
            acc = np.where(ok, (acc + prod).astype(f32), acc)   # one fp32 add
            ws = np.where(ok, (ws + wmin).astype(f32), ws)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = (acc * (f32(1.0) / ws).astype(f32)).astype(f32)
    # rows outside h0 < Y < h1 and uncovered pixels have ws == 0: the marker, as O.normalize's
    bits = np.where(ws == 0, MARKER_BITS, np.ascontiguousarray(out).view(np.uint32))
    return bits.astype(np.uint32).view(f32), ws


def fuse(emap, tiles, data, weights, abcd=None, out_w=M.OUT_W, out_h=M.OUT_H, zr=ZR):
    """u16 [out_h][out_w] of pf_fuse_weighted for one panorama."""
    data_nan = np.ascontiguousarray(staged(tiles, data, weights, abcd), f32)
    prev = buf = None
    for level in range(O.num_levels(out_w)):
        lv = O.level_dims(out_w, out_h, zr, level)
        lnorm, _ = weighted_targets(tiles, data_nan, weights, lv)
        buf = O.seed_level0(emap, lv) if level == 0 else O.upsample(prev, lv)
        buf = O.jacobi(buf, lnorm, lv, lv.iters)
        prev = buf
    return O.quantize(buf)


# ---- registration -----------------------------------------------------------------------------
def sample_elements(tile, emap, zr=ZR):
    """The element inside the tile that every registration sample reads: the samples of a tile
    that holds its own element indices, scaled into [0.25, 0.75) (inside the clamp range; the
    assertion checks that the indices read back exactly)."""
    n = tile.width * tile.height * tile.channels
    probe = np.zeros(tile.offset + n, f32)
    probe[tile.offset:] = (0.25 + 0.5 * np.arange(n, dtype=np.float64) / n).astype(f32)
    xs, _, _, _ = O.reg_samples(tile, probe, emap, zr)
    el = np.rint((xs - 0.25) * 2.0 * n).astype(np.int64)
    assert np.array_equal(probe[tile.offset + el].astype(np.float64), xs)
    return el


def reg_sums(xs, ys, w, used):
    """k_register_weighted's 16 sums of one tile: the 15 weighted moment sums and the count."""
    used = np.asarray(used, bool)
    T = M.reg_terms(np.where(used, xs, 0.5), np.where(used, ys, 0.5))
    W = np.where(used, np.asarray(w, f32).astype(np.float64), 0.0)
    T = np.where(used[:, None], W[:, None] * T, 0.0)
    T = np.concatenate([T, used[:, None].astype(np.float64)], 1)
    ns = T.shape[0]
    rows = (ns + M.LANES - 1) // M.LANES
    P = np.zeros((rows * M.LANES, 16), np.float64)
    P[:ns] = T
    P = P.reshape(rows, M.LANES, 16)
    part = np.zeros((M.LANES, 16), np.float64)
    for r in range(rows):
        part = part + P[r]
    stride = M.LANES // 2
    while stride >= 1:
        part[:stride] = part[:stride] + part[stride:2 * stride]
        stride //= 2
    return part[0].copy()


def register(tiles, data, weights, emap, zr=ZR):
    """(coeffs64 [n][4], summary [n][2] = {used samples, sum of w}, sums [n][16]) of every tile."""
    n = len(tiles)
    data = np.ascontiguousarray(data, f32)
    u = usable(weights).ravel()
    c64 = np.full((n, 4), np.nan, np.float64)
    summ = np.zeros((n, 2), np.float64)
    sums = np.zeros((n, 16), np.float64)
    for p in range(n):
        t = tiles[p]
        el = sample_elements(t, emap, zr)
        raw = data[t.offset + el]
        xs, ys, _, _ = O.reg_samples(t, data, emap, zr)
        w = u[t.offset + el]
        used = (w > 0) & np.isfinite(raw) & np.isfinite(ys)
        S = reg_sums(xs, ys, w, used)
        sums[p] = S
        summ[p] = (S[15], S[9])
        if S[15] >= 4:
            c, _ = O.lm_moments(S[:15])
            if np.isfinite(c).all():
                c64[p] = c
    return c64, summ, sums


def merge(emap, tiles, data, weights, out_w=M.OUT_W, zr=ZR):
    """(u16 [out_w / 2][out_w], abcd float32 [n][4]) of pf_merge_weighted for one panorama."""
    c64, _, _ = register(tiles, data, weights, emap, zr)
    abcd = c64.astype(f32)
    return fuse(emap, tiles, data, weights, abcd, out_w, out_w // 2, zr), abcd
