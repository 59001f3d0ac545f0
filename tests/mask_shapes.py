"""The cases of the tile-pixel validity rule beyond 512x256 C1: output sizes, hole sets, layouts.

TEST INFRASTRUCTURE ONLY: tests/test_mask_shapes.py proves every case on the CPU (the composition
of tests/mask_ref.py is the oracle where nothing is invalid, and every hole set lands where it is
meant to); tests/test_gpu_mask_shapes.py holds the library to the compositions, bit for bit.

Sizes.  ROWS are rows of test_fuse_shapes.SHAPES (imported, with the baselines that table pairs
them with) on the C1 layout:
  600x300    k_border's scalar path, partial patches on every level, ragged strips, odd height
  496x248    a strip wider than a row
  500x248    odd-width level 0 on sweeps, then the streamed upsample of an odd level
  440x220    narrow sweeps
  1096x500   height != width / 2
  1024x400   levels 0 and 1 resident by default
  2048x400   the 512-wide resident level by default
Under the rule no level has the certificate (level_full() is false), so expected_engines() with
certificate=False: sweeps where tcap < 1, else streamed / general; never resident, never packed.

Hole sets.  Defined on the fusion grid and mapped back to tile elements through the oracle's tap
indices (O.probe_taps per tile, clamped as the gather clamps them), so they land where they are
meant to at every size:
  seam      a tile-space rectangle of ONE tile under a grid rectangle that straddles the edge of
            its overlap with a neighbour: cover 2 -> 1 on one side, 1 -> 0 on the other
  bandrows  the centre taps of band rows h0+1 and h1-1 over a run of columns, on every level
  edgecols  the centre taps of a run of rows in the first and the last covered column, every level
  checker   a checkerboard of tile pixels (period one pixel) under 80 x 12 pixels of the finest
            level at columns 100..179: it crosses the 64 x 8 patch border at column 128, a patch
            row border, and the first strip border of every strip width (108..124)
  isolated  a region whose centre taps are invalid except the stencils of a sparse lattice of
            pixels: single valid pixels inside an invalid region
  tile      a whole tile
"""
import functools

import numpy as np

import mask_ref as M
import pf_synth
import pyoracle as O
import test_fuse_shapes as TS
import tile_shapes as TL

ZR = M.ZR
SEED = 20261020
SIZES = [(600, 300), (496, 248), (500, 248), (440, 220), (1096, 500), (1024, 400), (2048, 400)]
ROWS = [r for r in TS.SHAPES if (r[0], r[1]) in SIZES]
ROW_INDEX = {(r[0], r[1]): i for i, r in enumerate(TS.SHAPES)}
SETS = ["seam", "bandrows", "edgecols", "checker", "isolated", "tile"]
FULL_CHECKS = [(600, 300), (500, 248)]  # also fuse(pre-transformed) and fuse_check
BATCH_SIZES = [(600, 300), (1024, 400)]
LAYOUTS = ["LERES", "MIDAS", "MIXED", "LERES3", "MIDAS3"]
CHECKER = (100, 80, 12)  # first column, columns, rows of the checker region (finest level)


def size_id(s):
    return f"{s[0]}x{s[1]}"


class Case:
    """One layout with its inputs at one output size; everything is shared: copy before writing."""

    def __init__(self, name, lay, tiles, emap, data, out_w, out_h, channels=1):
        self.name, self.lay, self.tiles, self.emap = name, lay, tiles, emap
        self.data, self.out_w, self.out_h, self.channels = data, out_w, out_h, channels
        for a in (self.emap, self.data):
            a.setflags(write=False)
        self.nlevels = O.num_levels(out_w)

    def level(self, k):
        return O.level_dims(self.out_w, self.out_h, ZR, k)


def row_emap(i):
    """The baseline test_fuse_shapes pairs with row i of its table: BASELINES[i % 3]."""
    ew, eh, ec = TS.BASELINES[i % len(TS.BASELINES)]
    e = pf_synth.baseline_emap(pf_synth.seeds_for(1, SEED + 10 + i), ew, eh)[0].numpy()
    e = np.ascontiguousarray(e, np.float32)
    if ec == 1:
        return e
    rest = np.random.RandomState(SEED % (1 << 31) + i).rand(eh, ew, ec - 1).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([e[..., None], rest], -1))


@functools.lru_cache(maxsize=None)
def row_case(size):
    """C1 (six 256 x 256 tiles of the default scene) at a size of ROWS."""
    lay, tiles, _, data = M.c1_inputs()
    return Case(size_id(size), lay, tiles, row_emap(ROW_INDEX[size]), np.array(data), *size)


@functools.lru_cache(maxsize=None)
def layout_case(name):
    """The other layouts at 512 x 256: tile_shapes.channel_case's LeReS 64x48 and MiDaS 40x30
    (one channel, and three with channels 1-2 at -7) and the mixed off-grid C1 sizes."""
    if name == "MIXED":
        lay = TL.layout_with(TL.MIXED_SIZES)
        tiles, total = O.make_tiles(lay)
        seeds = pf_synth.seeds_for(1, SEED)
        emap = pf_synth.baseline_emap(seeds, TL.EW, TL.EW // 2)[0].numpy()
        gt = pf_synth.scene_depth(seeds, TL.OUT_W, TL.OUT_W // 2)[0].numpy()
        data = O.warp_depth(gt, tiles, total, O.responses(pf_synth.responses(seeds, lay.ntiles)))
        return Case(name, lay, tiles, np.array(emap, np.float32), data, M.OUT_W, M.OUT_H)
    k = TL.channel_case(name[:5])
    three = name.endswith("3")
    return Case(name, k["lay"], k["t3"] if three else k["t1"], np.array(k["emaps"][0]),
                np.array((k["d3"] if three else k["d1"])[0]), M.OUT_W, M.OUT_H,
                3 if three else 1)


@functools.lru_cache(maxsize=None)
def abcd(case):
    """The oracle's unmasked registration of the case's tiles: float32 [ntiles][4]."""
    if case.lay is M.c1_inputs()[0]:
        return M.c1_abcd()  # against C1's own 128 x 64 baseline
    _, c = O.merge(case.emap, case.tiles, np.array(case.data), case.out_w, ZR)
    return c


# ---- the oracle's tap maps, per tile ------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def tile_maps(case, level):
    """Per tile (inbox bool [h][w], taps int64 [h][w][5], clamped bool [h][w][5]): the pixels of
    the tile's box, the element index inside the tile that each of their five taps reads (clamped
    as pfo_targets and the gather clamp it) and which taps were clamped."""
    lv = case.level(level)
    zeros = np.zeros(sum(t.width * t.height * t.channels for t in case.tiles), np.float32)
    res = []
    for p, t in enumerate(case.tiles):
        one = (O.Tile * 1)()
        one[0] = t
        raw = O.probe_taps(one, lv).astype(np.int64)
        _, c = O.targets_subset(case.tiles, p, p + 1, zeros, lv)
        n = t.width * t.height * t.channels
        out = (raw < 0) | (raw >= n)
        taps = np.where(raw < 0, 0, np.where(raw >= n, n - t.channels, raw))
        res.append((c > 0, taps, out & (c > 0)[..., None]))
    return res


def cover(case, level):
    return sum(m[0].astype(np.int32) for m in tile_maps(case, level))


def _centres(case, level, sel):
    """[(p, elements)]: the centre taps of the grid pixels `sel` in every tile that covers them."""
    return [(p, np.unique(taps[..., 2][sel & inbox]))
            for p, (inbox, taps, _) in enumerate(tile_maps(case, level)) if (sel & inbox).any()]


def _tile_bbox(t, idx):
    """(ys, xs) index grids of the tile-space bounding box of elements idx."""
    px = np.asarray(idx) // t.channels
    ty, tx = px // t.width, px % t.width
    return np.meshgrid(np.arange(ty.min(), ty.max() + 1), np.arange(tx.min(), tx.max() + 1),
                       indexing="ij")


def _band(lv):
    b = np.zeros((lv.h, lv.w), bool)
    b[lv.h0 + 1:lv.h1] = True
    return b


def holes_seam(case):
    fin = case.nlevels - 1
    lv = case.level(fin)
    cov = cover(case, fin)
    band = _band(lv)
    for p, (inbox, taps, _) in enumerate(tile_maps(case, fin)):
        both, only = inbox & (cov == 2) & band, inbox & (cov == 1) & band
        near = np.zeros_like(both)
        near[:, 1:] |= both[:, :-1]
        near[:, :-1] |= both[:, 1:]
        near[1:] |= both[:-1]
        near[:-1] |= both[1:]
        ys, xs = np.nonzero(only & near)
        if ys.size == 0:
            continue
        cy, cx = (c.mean() for c in np.nonzero(inbox))
        k = int(np.argmin((ys - cy) ** 2 + (xs - cx) ** 2))
        ry, rx = max(8, lv.h // 12), max(12, lv.w // 20)
        sel = np.zeros_like(both)
        sel[max(ys[k] - ry, 0):ys[k] + ry + 1, max(xs[k] - rx, 0):xs[k] + rx + 1] = True
        t = case.tiles[p]
        gy, gx = _tile_bbox(t, taps[..., 2][sel & inbox])
        return [(p, ((gy * t.width + gx) * t.channels).ravel())]
    raise AssertionError("no tile with a two-tile seam")


def holes_bandrows(case):
    res = []
    for level in range(case.nlevels):
        lv = case.level(level)
        sel = np.zeros((lv.h, lv.w), bool)
        x0 = lv.w // 8
        for y in (lv.h0 + 1, lv.h1 - 1):
            sel[y, x0:x0 + max(16, lv.w // 6)] = True
        res += _centres(case, level, sel)
    return res


def holes_edgecols(case):
    res = []
    for level in range(case.nlevels):
        lv = case.level(level)
        cols = np.flatnonzero(cover(case, level)[lv.h0 + 1] > 0)
        mid, half = (lv.h0 + lv.h1) // 2, max(4, lv.h // 10)
        sel = np.zeros((lv.h, lv.w), bool)
        sel[mid - half:mid + half, [cols[0], cols[-1]]] = True
        res += _centres(case, level, sel)
    return res


def holes_checker(case):
    fin = case.nlevels - 1
    lv = case.level(fin)
    x0, nx, ny = CHECKER
    y0 = (lv.h0 + lv.h1) // 2 - ny // 2
    assert x0 + nx <= lv.w and lv.h0 < y0 and y0 + ny < lv.h1
    sel = np.zeros((lv.h, lv.w), bool)
    sel[y0:y0 + ny, x0:x0 + nx] = True
    res = []
    for p, (inbox, taps, _) in enumerate(tile_maps(case, fin)):
        if not (sel & inbox).any():
            continue
        t = case.tiles[p]
        gy, gx = _tile_bbox(t, taps[..., 2][sel & inbox])
        odd = (gy + gx) % 2 == 0
        res.append((p, ((gy * t.width + gx) * t.channels)[odd]))
    return res


def holes_isolated(case, level=None):
    """At `level` (default: the finest level at which it works, found by test_mask_shapes): a
    region of 40 x 16 pixels under the band's middle; the pixels on a lattice of period 6 keep
    their five taps, every other centre tap of the region is invalid."""
    if level is None:
        level = isolated_level(case)
    lv = case.level(level)
    nx, ny = min(40, lv.w // 3), min(16, (lv.h1 - lv.h0) // 3)
    x0, y0 = lv.w // 2 - nx // 2, (lv.h0 + lv.h1) // 2 + 2
    Y, X = np.mgrid[0:lv.h, 0:lv.w]
    region = (X >= x0) & (X < x0 + nx) & (Y >= y0) & (Y < y0 + ny)
    keep = region & ((X - x0) % 6 == 3) & ((Y - y0) % 6 == 3)
    plus = keep.copy()
    plus[:, 1:] |= keep[:, :-1]
    plus[:, :-1] |= keep[:, 1:]
    plus[1:] |= keep[:-1]
    plus[:-1] |= keep[1:]
    res = []
    for p, (inbox, taps, _) in enumerate(tile_maps(case, level)):
        if not (region & inbox).any():
            continue
        bad = np.setdiff1d(taps[..., 2][region & ~plus & inbox], taps[keep & inbox].ravel())
        res.append((p, bad))
    return res


@functools.lru_cache(maxsize=None)
def isolated_level(case):
    """The finest level at which holes_isolated leaves an isolated valid pixel (a level finer than
    the tiles maps several pixels to one tile pixel: none can stay valid alone)."""
    for level in range(case.nlevels - 1, -1, -1):
        d = M.apply_holes(case.tiles, case.data, holes_isolated(case, level))
        lv = case.level(level)
        _, cnt, cov = M.masked_targets(case.tiles, d, lv, None)
        if M.level_stats(cnt, cov, lv)["isolated"] > 0:
            return level
    raise AssertionError(f"{case.name}: no level keeps an isolated valid pixel")


def holes_tile(case):
    p = min(M.ALL_TILE, len(case.tiles) - 1)
    t = case.tiles[p]
    return [(p, np.arange(t.width * t.height) * t.channels)]


def holes_clamped(case):
    """One hole under a *clamped* tap of level 0: the element the clamp lands on, in the first
    tile that has one."""
    for p, (_, taps, clamped) in enumerate(tile_maps(case, 0)):
        if clamped.any():
            return [(p, np.unique(taps[clamped])[:1])]
    raise AssertionError(f"{case.name}: no clamped tap at level 0")


BUILDERS = {"seam": holes_seam, "bandrows": holes_bandrows, "edgecols": holes_edgecols,
            "checker": holes_checker, "isolated": holes_isolated, "tile": holes_tile,
            "clamped": holes_clamped, "none": lambda case: []}


@functools.lru_cache(maxsize=None)
def holes(case, name):
    return BUILDERS[name](case)


def raw(case, name):
    """The case's raw tile data with NaN at the holes of set `name`: a copy."""
    return M.apply_holes(case.tiles, case.data, holes(case, name))


@functools.lru_cache(maxsize=None)
def composition(case, name, cover_limit=2):
    """(u16 panorama, stats) of the masked fusion of raw(case, name) under abcd(case): the
    reference of fuse(raw, coeffs), fuse(transformed) and fuse_check.  Computed once."""
    d = M.transform(case.tiles, raw(case, name), abcd(case))
    return M.masked_fuse(case.emap, case.tiles, d, case.out_w, case.out_h, ZR, cover_limit)


def stats(case, name, cover_limit=2):
    """masked_fuse's stats of a set without the solve."""
    d = M.transform(case.tiles, raw(case, name), abcd(case))
    return M.masked_stats(case.tiles, d, case.out_w, case.out_h, ZR, cover_limit)


def expected_engines(case):
    """[engine] per level under the rule: sweeps where tcap < 1, else streamed; all general."""
    got = TS.expected_engines(case.tiles, np.array(case.data), case.out_w, case.out_h,
                              certificate=False)
    assert all(form == "general" and engine != "resident" for engine, form in got)
    return [engine for engine, _ in got]


def max_cover(case):
    return max(int(cover(case, k).max()) for k in range(case.nlevels))


def cover_limit(case):
    """2 where the composition is order-free and proven against the oracle; None where the layout
    covers a pixel more than twice (the sum then restates targets_patch's ascending order)."""
    return 2 if max_cover(case) <= 2 else None


# ---- registration: tiles left with an exact number of valid samples ----------------------------
def sample_elements(case, p):
    """int64 [ns]: the tile element each registration sample of tile p reads, from O.reg_samples
    on tiles that hold their own element index (as (e + 1) / (n + 2), inside the clamp range)."""
    t = case.tiles[p]
    n = t.width * t.height * t.channels
    assert n + 2 < 1 << 20
    code = np.zeros(case.data.size, np.float32)
    code[t.offset:t.offset + n] = (np.arange(n) + 1.0) / (n + 2.0)
    xs, _, _, _ = O.reg_samples(t, code, case.emap, ZR)
    e = np.rint(xs * (n + 2.0) - 1.0).astype(np.int64)
    assert ((e >= 0) & (e < n)).all() and (e % t.channels == 0).all()
    assert np.array_equal(code[t.offset + e].astype(np.float64), xs), "the code must decode"
    return e


def holes_keep_samples(case, p, keep):
    """Tile p with every sampled element invalid except some that `keep` samples read in all
    (several samples may read one element): exactly `keep` valid samples."""
    import itertools
    e = sample_elements(case, p)
    val, counts = np.unique(e, return_counts=True)
    pool = [(int(v), int(c)) for c in range(1, keep + 1) for v in val[counts == c][:keep]]
    for r in range(1, keep + 1):
        for combo in itertools.combinations(pool, r):
            if sum(c for _, c in combo) == keep:
                return [(p, np.setdiff1d(val, [v for v, _ in combo]))]
    raise AssertionError(f"{case.name} tile {p}: no elements read by exactly {keep} samples")


REG_TILES = {"empty": 4, "three": 1, "four": 2}  # which tile of a six-tile layout gets what


def reg_holes(case):
    """The registration case: an all-invalid tile, a tile with exactly 3 and one with exactly 4
    valid samples, and the seam rectangle wherever it falls."""
    return (holes_tile(case) + holes_keep_samples(case, REG_TILES["three"], 3)
            + holes_keep_samples(case, REG_TILES["four"], 4) + holes(case, "seam"))


# ---- stitch -------------------------------------------------------------------------------------
STITCH_SIZES = [(100, 50), (101, 51)]


def stitch_maps(tiles, W, H):
    """(inside bool [n][H][W], elements int64 [n][H][W]): per tile the pixels its box holds and the
    (clamped) tile element the stitch samples there."""
    import stitch_ref as SR
    X = np.arange(W)[None, :]
    Y = np.arange(H)[:, None]
    ins, els = [], []
    for (x0, x1, y0, y1), t in zip(SR.boxes(tiles, W, H), tiles):
        ins.append((X >= min(x0, x1)) & (X <= max(x0, x1)) & (Y >= y0) & (Y <= y1))
        idx = SR.tile_indices(t, W, H)
        lim = t.width * t.height * t.channels
        idx = np.where(idx < 0, 0, idx)
        els.append(np.where(idx >= lim, lim - t.channels, idx))
    return np.stack(ins), np.stack(els)


def stitch_holes(tiles, W, H):
    """(holes, third): the elements the first candidate tile samples under a W/8 x H/4 block in
    the middle of tile 0's box, and -- where some pixel lies in three boxes -- the elements its
    first two candidates sample there; third = (y, x, tile) of that pixel's third candidate, or
    None where the layout has no such pixel at this size."""
    ins, els = stitch_maps(tiles, W, H)
    ys, xs = np.nonzero(ins[0])
    cy, cx = int(ys.mean()), int(xs.mean())
    block = np.zeros((H, W), bool)
    block[cy - H // 8:cy + H // 8, cx - W // 16:cx + W // 16] = True
    res = [(0, np.unique(els[0][block & ins[0]]))]
    third = None
    deep = np.argwhere(ins.sum(0) >= 3)
    if deep.size:
        y, x = (int(v) for v in deep[len(deep) // 2])
        cand = np.flatnonzero(ins[:, y, x])
        res += [(int(p), np.array([els[p, y, x]])) for p in cand[:2]]
        third = (y, x, int(cand[2]))
    return res, third
