"""CPU reference of the tile-pixel validity rule (pf_set_tile_validity), composed from the
oracle's own building blocks.

TEST INFRASTRUCTURE ONLY.  tests/test_mask_ref.py proves the compositions against the oracle on
unmasked inputs (bit for bit); tests/test_gpu_mask.py holds the library to them.  The functions
take any layout, tile data, channel count and output size: tests/mask_shapes.py builds the cases
beyond 512x256 C1 on them (apply_holes, masked_targets, level_stats), tests/test_mask_shapes.py
proves those, tests/test_gpu_mask_shapes.py runs them.  HOLES, with_holes and the c1_* caches are
the C1 case of tests/test_gpu_mask.py.

Fusion.  Per level and tile p, O.targets_subset(tiles, p, p + 1, data, lv) on tile data that
carries NaN at every invalid pixel: a NaN tap poisons exactly the stencils that read it, so tile p
is valid at a pixel iff its count is positive and its sum is not NaN.  The valid tiles' sums are
added in tile order and counted, then O.normalize, O.seed_level0 / O.upsample, O.jacobi and
O.quantize run as in pfo_solve_depth_all.  Exact as long as no pixel is covered by more than two
tiles (a + b is one rounding whatever the order; the oracle's own statement, pf_oracle.c:472):
masked_fuse asserts it.

Registration.  k_register's sums restated: lane l of 256 adds the 15 terms of samples l, l + 256,
... in order from 0.0, then the halving tree 128 ... 1; a skipped sample's terms are 0.0, and all
terms are positive, so adding 0.0 changes no bit.  The sums go to O.lm_moments.

Stitch.  The first tile in ascending order whose box holds the pixel and whose sampled value is
valid, from tests/stitch_ref.py's boxes and indices.
"""
import functools

import numpy as np

import pf_layouts as PL
import pf_synth
import pyoracle as O
import stitch_ref as SR

f32 = np.float32
ZR = PL.ZENITH_RANGE
OUT_W, OUT_H = 512, 256
TILE = 256
LANES = 256
# the issue's holes at C1: a rectangle of tile 0 that crosses the row shared by two tiles and
# several 64 x 8 patch borders, a whole tile, one pixel
RECT = (0, slice(100, 256), slice(100, 180))
ALL_TILE = 4
PIXEL = (0, 131, 91)  # a pixel that the two finer levels sample (five stencils each)
HOLES = {
    "rect": [RECT],
    "tile": [(ALL_TILE, slice(0, TILE), slice(0, TILE))],
    "pixel": [(PIXEL[0], slice(PIXEL[1], PIXEL[1] + 1), slice(PIXEL[2], PIXEL[2] + 1))],
    "none": [],
}


@functools.lru_cache(maxsize=None)
def c1_inputs():
    """(layout, oracle tiles, emap [64][128], raw tile data [6 * 256 * 256]) at C1, the default
    seed; the arrays are shared: copy before writing."""
    lay = PL.config_layout("C1")
    seeds = pf_synth.seeds_for(1)
    emap = pf_synth.baseline_emap(seeds, 128, 64)[0].numpy()
    gt = pf_synth.scene_depth(seeds, OUT_W, OUT_H)[0].numpy()
    tiles, total = O.make_tiles(lay)
    resp = pf_synth.responses(seeds, lay.ntiles)
    data = O.warp_depth(gt, tiles, total, O.responses(resp))
    emap.setflags(write=False)
    data.setflags(write=False)
    return lay, tiles, emap, data


def with_holes(data, name, value=np.nan):
    """A copy of the C1 tile data with the holes of HOLES[name] written as `value`."""
    d = np.array(data, np.float32).reshape(-1, TILE, TILE)
    for p, ys, xs in HOLES[name]:
        d[p, ys, xs] = value
    return d.reshape(-1)


def transform(tiles, data, abcd):
    """Depth2DepthTransform of every tile (the oracle's), NaN kept: a copy."""
    d = np.array(data, np.float32)
    for p in range(len(tiles)):
        O.depth_to_depth(tiles[p], d, abcd[p])
    return d


# ---- registration -----------------------------------------------------------------------------
def reg_terms(xs, ys):
    """The 15 terms of every sample, fp64 [ns][15], as pf_kernels.hip / pf_oracle.c form them."""
    X = np.asarray(xs, np.float64)
    y = np.asarray(ys, np.float64)
    X2 = X * X
    X3 = X * X * X
    return np.stack([X3 * X3, X3 * X2, X3 * X, X3, X2 * X2, X2 * X, X2, X * X, X,
                     np.ones_like(X), X3 * y, X2 * y, X * y, y, y * y], 1)


def reg_sums(xs, ys, valid=None):
    """k_register's 15 sums of one tile; valid [ns] bool (None: all): a skipped sample adds 0.0."""
    T = reg_terms(np.where(valid, xs, 0.5) if valid is not None else xs,
                  np.where(valid, ys, 0.5) if valid is not None else ys)
    if valid is not None:
        T = np.where(np.asarray(valid, bool)[:, None], T, 0.0)
    ns = T.shape[0]
    rows = (ns + LANES - 1) // LANES
    P = np.zeros((rows * LANES, 15), np.float64)
    P[:ns] = T
    P = P.reshape(rows, LANES, 15)
    part = np.zeros((LANES, 15), np.float64)
    for r in range(rows):  # lane l: samples l, l + 256, ... in order
        part = part + P[r]
    stride = LANES // 2
    while stride >= 1:
        part[:stride] = part[:stride] + part[stride:2 * stride]
        stride //= 2
    return part[0].copy()


def tile_samples(tiles, data_nan, emap, p):
    """(xs, ys, valid) of tile p: the clamped samples and which of them the rule keeps, from tile
    data that carries NaN at the invalid pixels (a NaN stays NaN through the clamp)."""
    xs, ys, _, _ = O.reg_samples(tiles[p], np.ascontiguousarray(data_nan, np.float32), emap, ZR)
    valid = ~np.isnan(xs) & np.isfinite(ys)
    return xs, ys, valid


def register(tiles, data_nan, emap):
    """(coeffs64 [n][4], sums [n][15], valid sample counts [n]) of every tile alone; a tile with
    fewer than 4 valid samples, or a non-finite solution, gets NaN."""
    n = len(tiles)
    c64 = np.full((n, 4), np.nan, np.float64)
    sums = np.zeros((n, 15), np.float64)
    cnt = np.zeros(n, np.int64)
    for p in range(n):
        xs, ys, valid = tile_samples(tiles, data_nan, emap, p)
        sums[p] = reg_sums(xs, ys, valid)
        cnt[p] = int(valid.sum())
        if cnt[p] >= 4:
            c, _ = O.lm_moments(sums[p])
            if np.isfinite(c).all():
                c64[p] = c
    return c64, sums, cnt


def register_joint(sums, active):
    """The joint solve: the active tiles' sums added in tile order from 0.0, then the LM."""
    S = np.zeros(15, np.float64)
    for p in active:
        S = S + sums[p]
    if S[9] < 4:
        return np.full(4, np.nan)
    c, _ = O.lm_moments(S)
    return c if np.isfinite(c).all() else np.full(4, np.nan)


# ---- fusion -----------------------------------------------------------------------------------
PATCH_W, PATCH_H = 64, 8  # kTPW, kTPH (csrc/pf_targets.hip): a block's patch of band pixels
# every strip width V = 128 - 2 * Tp of the streamed Jacobi passes (csrc/pf_ctx.hpp
# strip_geometry: Tp = the pass depth 1..10 rounded up to even)
STRIP_WIDTHS = (124, 120, 116, 112, 108)


def apply_holes(tiles, data, holes, value=np.nan):
    """A copy of `data` (any layout, size and channel count) with `value` at the elements of
    `holes`: [(tile p, element indices inside tile p)]."""
    d = np.array(data, np.float32).ravel()
    for p, idx in holes:
        d[tiles[p].offset + np.asarray(idx, np.int64)] = value
    return d


def masked_targets(tiles, data_nan, lv, cover_limit=2):
    """(Lsum, cnt, cover) of one level: the valid tiles' sums added in ascending tile order, how
    many there were, and the layout's cover.  cover_limit None lifts the cover-of-two condition:
    the ascending order is then targets_patch's order restated, not derived from the oracle."""
    Lsum = np.zeros((lv.h, lv.w), np.float32)
    cnt = np.zeros((lv.h, lv.w), np.int32)
    cover = np.zeros((lv.h, lv.w), np.int32)
    for p in range(len(tiles)):
        s, c = O.targets_subset(tiles, p, p + 1, data_nan, lv)
        ok = (c > 0) & ~np.isnan(s)
        with np.errstate(invalid="ignore"):
            Lsum = np.where(ok, Lsum + s, Lsum).astype(np.float32)
        cnt += ok
        cover += c > 0
    if cover_limit is not None:
        assert cover.max() <= cover_limit, "the composition is exact only up to a cover of two"
    return Lsum, cnt, cover


def level_stats(cnt, cover, lv):
    """What the holes did to one level.  `dropped`: pixels whose cover went from 2 to 1;
    `unwindowed`: covered band pixels left without a valid tile (they carry the marker);
    `max_cover`; `unwindowed_first_row` / `_last_row`: those on band rows h0+1 / h1-1;
    `unwindowed_first_col` / `_last_col`: those in the first / last covered column of row h0+1;
    `unwindowed_patches`: the 64 x 8 target patches that hold one; `strip_seams`: the strip widths
    V of STRIP_WIDTHS with one in columns k*V - 1 and k*V for some k >= 1; `isolated`: pixels with
    a valid tile whose four neighbours have none."""
    band = np.zeros((lv.h, lv.w), bool)
    band[lv.h0 + 1:lv.h1] = True
    un = (cover > 0) & (cnt == 0) & band
    cols = np.flatnonzero(cover[lv.h0 + 1] > 0)
    ys, xs = np.nonzero(un)
    patches = set(zip(((ys - lv.h0) // PATCH_H).tolist(), (xs // PATCH_W).tolist()))
    ucol = un.any(0)
    seams = [V for V in STRIP_WIDTHS
             if any(ucol[b - 1] and ucol[b] for b in range(V, lv.w, V))]
    ok = (cnt > 0) & band
    none = np.pad(cnt == 0, 1, constant_values=False)
    iso = ok & none[1:-1, :-2] & none[1:-1, 2:] & none[:-2, 1:-1] & none[2:, 1:-1]
    return {"dropped": int(((cover == 2) & (cnt == 1) & band).sum()),
            "unwindowed": int(un.sum()),
            "max_cover": int(cover.max()),
            "unwindowed_first_row": int(un[lv.h0 + 1].sum()),
            "unwindowed_last_row": int(un[lv.h1 - 1].sum()),
            "unwindowed_first_col": int(un[:, cols[0]].sum()) if cols.size else 0,
            "unwindowed_last_col": int(un[:, cols[-1]].sum()) if cols.size else 0,
            "unwindowed_patches": len(patches),
            "strip_seams": seams,
            "isolated": int(iso.sum())}


def masked_stats(tiles, data_nan, out_w=OUT_W, out_h=OUT_H, zr=ZR, cover_limit=2):
    """masked_fuse's stats alone (no solve): one level_stats per level."""
    data_nan = np.ascontiguousarray(data_nan, np.float32)
    stats = []
    for level in range(O.num_levels(out_w)):
        lv = O.level_dims(out_w, out_h, zr, level)
        _, cnt, cover = masked_targets(tiles, data_nan, lv, cover_limit)
        stats.append(level_stats(cnt, cover, lv))
    return stats


def masked_fuse(emap, tiles, data_nan, out_w=OUT_W, out_h=OUT_H, zr=ZR, cover_limit=2):
    """(u16 [out_h][out_w], stats) of the masked fusion; stats: level_stats() per level."""
    data_nan = np.ascontiguousarray(data_nan, np.float32)
    stats = []
    prev = None
    buf = None
    for level in range(O.num_levels(out_w)):
        lv = O.level_dims(out_w, out_h, zr, level)
        Lsum, cnt, cover = masked_targets(tiles, data_nan, lv, cover_limit)
        stats.append(level_stats(cnt, cover, lv))
        Lnorm = O.normalize(Lsum, cnt, lv)
        buf = O.seed_level0(emap, lv) if level == 0 else O.upsample(prev, lv)
        buf = O.jacobi(buf, Lnorm, lv, lv.iters)
        prev = buf
    return O.quantize(buf), stats


@functools.lru_cache(maxsize=None)
def c1_abcd():
    """The unmasked C1 registration (the oracle's merge): float32 [6][4]."""
    _, tiles, emap, data = c1_inputs()
    _, abcd = O.merge(emap, tiles, np.array(data), OUT_W, ZR)
    return abcd


@functools.lru_cache(maxsize=None)
def c1_masked(name):
    """(u16 result, stats) of the masked C1 fusion under c1_abcd() with the holes HOLES[name]:
    the reference of both fuse(raw tiles with NaN, coeffs) and fuse(transformed tiles with NaN)."""
    _, tiles, emap, data = c1_inputs()
    return masked_fuse(emap, tiles, transform(tiles, with_holes(data, name), c1_abcd()))


# ---- stitch -----------------------------------------------------------------------------------
def stitch_valid(tiles, data_nan, W, H, coeffs=None):
    """u16 [H][W]: per pixel the first tile whose box holds it and whose sampled value is valid
    (not NaN raw; finite after the transform), 0 under none."""
    data_nan = np.asarray(data_nan, np.float32).ravel()
    X = np.arange(W)[None, :]
    Y = np.arange(H)[:, None]
    out = np.zeros((H, W), np.uint16)
    done = np.zeros((H, W), bool)
    for p, ((x0, x1, y0, y1), t) in enumerate(zip(SR.boxes(tiles, W, H), tiles)):
        inside = (X >= min(x0, x1)) & (X <= max(x0, x1)) & (Y >= y0) & (Y <= y1)
        idx = SR.tile_indices(t, W, H)
        lim = t.width * t.height * t.channels
        idx = np.where(idx < 0, 0, idx)
        idx = np.where(idx >= lim, lim - t.channels, idx)
        raw = data_nan[t.offset + idx]
        v = SR.cubic_map(raw, coeffs[p]).reshape(raw.shape) if coeffs is not None else raw
        take = inside & ~done & ~np.isnan(raw) & np.isfinite(v)
        out[take] = SR.quantize(v[take])
        done |= take
    return out
