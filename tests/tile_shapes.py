"""Tile shapes no other test runs: off-grid sizes, layouts of mixed sizes, interleaved channels.

The cases and helpers of tests/test_tile_shapes.py (CPU) and tests/test_gpu_tile_shapes.py (GPU).

* ``MIXED_SIZES`` on the C1 windows: six tiles of six sizes, none a whole number of the depth
  warp's 64 x 32 patches.  ``classify`` restates, in numpy from ``panofuse.warp_coords`` (the
  host probe), how ``warp_patches_host`` (pw % 4 == 0: ragged 16-B units) and ``k_patch_box``
  (else: the bounding box) send each patch to one of ``PATHS``, and whether the patch is cut by
  the tile's right edge (x), its bottom edge (y), both (xy) or not at all (full).
  ``cut_condition`` is the coverage claim of the GPU test: over ``PANOS`` every path runs a
  patch cut in X and a patch cut in Y.
* ``warp_depth_gather``: the depth warp without a response as a float32 numpy gather from the
  same map, in the oracle's operand order -- a checker that shares no code with it.
* ``SMALL_SIZES``: the smallest tiles ``pf_set_tiles`` accepts, and one pixel past a patch.
* ``RGB_SIZES``: widths that are multiples of 4 but not of the RGB warp's 64-pixel patch, so the
  LDS-staged kernel runs partial columns; ``RGB_SIZES_UNALIGNED`` has one width of 66, which
  sends the whole layout to the per-pixel kernel.
* ``interleave`` / ``FILL``: 3-channel tile data whose channel 0 is the 1-channel data and whose
  other channels hold ``FILL``.
"""
import collections

import numpy as np

import panofuse
import pf_layouts as PL

PATCH_W, PATCH_H = 64, 32  # kPatch, kPatchH (csrc/pf_warp.hip)
CAP = 4096  # kCap: LDS floats per staged footprint
LANES = 256  # kWB: threads per block = staging units per load slot

PANOS = [(512, 256), (300, 150), (302, 151), (1024, 512), (1022, 511)]
PATHS = ["rag-NS1", "rag-NS2", "rag-NS4", "rag-wide", "box-NS4", "box-NS8", "box-NS16", "box-wide"]
KINDS = ["full", "x", "y", "xy"]

MIXED_SIZES = [(100, 70), (65, 33), (63, 31), (130, 97), (200, 50), (40, 20)]
# 2x2 is the documented minimum; 64x2 one whole patch column, 65x2 one pixel past it; 2x33 one
# row past a patch; 3x3 the smallest odd square
SMALL_SIZES = [(2, 2), (3, 2), (64, 2), (65, 2), (2, 33), (3, 3)]
RGB_SIZES = [(100, 70), (68, 33), (4, 2), (132, 97), (200, 50), (40, 20)]
RGB_SIZES_UNALIGNED = [(100, 70), (66, 33), (4, 2), (132, 97), (200, 50), (40, 20)]

FILL = np.float32(-7.0)  # what channels 1.. of a multi-channel tile hold, before and after

# The existing table of tests/test_gpu_parity.py::test_warp_depth_ragged_batch_and_resize: plain
# C1 (256 x 256 tiles), patches per path in the order of PATHS.
C1_TABLE = {
    (512, 256): (108, 24, 60, 0, 0, 0, 0, 0),
    (300, 150): (144, 48, 0, 0, 0, 0, 0, 0),
    (302, 151): (0, 0, 0, 0, 132, 24, 36, 0),
    (1024, 512): (0, 96, 20, 76, 0, 0, 0, 0),
    (1022, 511): (0, 0, 0, 0, 0, 36, 60, 96),
}


def layout_with(sizes, base="C1"):
    """The windows of `base`, tile p of size sizes[p]."""
    lay = PL.config_layout(base)
    assert len(sizes) == lay.ntiles
    lay.tile_w = np.array([s[0] for s in sizes], np.int32)
    lay.tile_h = np.array([s[1] for s in sizes], np.int32)
    lay.name = f"{base}:" + ",".join(f"{w}x{h}" for w, h in sizes)
    return lay


def one_tile(lay, p):
    """Tile p of lay as a layout of its own."""
    return PL.Layout(f"{lay.name}[{p}]", lay.fovs[p:p + 1].copy(), lay.ranges[p:p + 1].copy(),
                     lay.tile_w[p:p + 1].copy(), lay.tile_h[p:p + 1].copy())


def tile_elems(lay, channels=1):
    return int(sum(int(w) * int(h) for w, h in zip(lay.tile_w, lay.tile_h))) * channels


def tile_slices(lay, channels=1):
    """Per tile the slice of its elements inside one panorama's tile block."""
    out, off = [], 0
    for w, h in zip(lay.tile_w, lay.tile_h):
        n = int(w) * int(h) * channels
        out.append(slice(off, off + n))
        off += n
    return out


def _wrap(d, pw):
    d = np.where(d > pw // 2, d - pw, d)
    return np.where(d < -(pw // 2), d + pw, d)


def _ragged_path(x0, y0, rx, pw, ph):
    """warp_patches_host: per panorama row of the footprint the 16-B units over the columns its
    corners read; wide when a row spans more than pw/2, the rows exceed ph, or the units 1024."""
    du = _wrap(x0 - rx, pw)
    vmin = int(y0.min())
    nv = int(y0.max()) - vmin + 2
    if nv > ph:
        return "rag-wide"
    nu = 0
    for r in range(nv):
        sel = (y0 - vmin == r) | (y0 - vmin == r - 1)
        if not sel.any():
            continue
        lo, hi = int(du[sel].min()), int(du[sel].max()) + 1
        if hi - lo + 1 > pw // 2:
            return "rag-wide"
        nu += (rx + hi + 4) // 4 - (rx + lo) // 4  # floor division, as floor_div
    if nu > CAP // 4:
        return "rag-wide"
    nq = -(-nu // LANES)
    return "rag-NS%d" % (1 if nq <= 1 else 2 if nq <= 2 else 4)


def _box_path(x0, y0, rx, pw):
    """k_patch_box: the azimuth-unwrapped bounding box of the corners, + 1 row and column."""
    du = _wrap(x0 - rx, pw)
    bw = int(du.max()) - int(du.min()) + 2
    bh = int(y0.max()) - int(y0.min()) + 2
    if bw * bh > CAP or bw > pw // 2:
        return "box-wide"
    ns = -(-(bw * bh) // LANES)
    return "box-NS%d" % (4 if ns <= 4 else 8 if ns <= 8 else 16)


def classify(lay, pw, ph):
    """Counter {(path, kind): patches} of the depth warp of lay on a pw x ph panorama."""
    out = collections.Counter()
    for p in range(lay.ntiles):
        w, h = int(lay.tile_w[p]), int(lay.tile_h[p])
        wxy, _ = panofuse.warp_coords(lay.fovs[p], w, h, pw, ph)
        m = wxy.reshape(h, w)
        x0 = (m & 0xFFFF).astype(np.int64)
        y0 = (m >> 16).astype(np.int64)
        for Y0 in range(0, h, PATCH_H):
            for X0 in range(0, w, PATCH_W):
                X1, Y1 = min(w, X0 + PATCH_W), min(h, Y0 + PATCH_H)
                kind = ("x" if X1 - X0 < PATCH_W else "") + ("y" if Y1 - Y0 < PATCH_H else "")
                xs, ys = x0[Y0:Y1, X0:X1].ravel(), y0[Y0:Y1, X0:X1].ravel()
                rx = int(x0[Y0, X0])
                path = _ragged_path(xs, ys, rx, pw, ph) if pw % 4 == 0 else _box_path(xs, ys, rx, pw)
                out[(path, kind or "full")] += 1
    return out


def path_counts(counter):
    """Patches per path, in the order of PATHS."""
    return tuple(sum(v for (path, _), v in counter.items() if path == name) for name in PATHS)


def classification_table(sizes, panos=PANOS):
    return {p: classify(layout_with(sizes), *p) for p in panos}


def format_table(table):
    lines = []
    for (pw, ph), c in table.items():
        cells = []
        for path in PATHS:
            kinds = [f"{k}{c[(path, k)]}" for k in KINDS if c[(path, k)]]
            if kinds:
                cells.append(f"{path}: " + " ".join(kinds))
        lines.append(f"{pw}x{ph} | " + " . ".join(cells))
    return "\n".join(lines)


def cut_condition(table):
    """Per path: does some panorama size run a patch cut in X, and one cut in Y, on it?"""
    got = {}
    for path in PATHS:
        x = sum(c[(path, "x")] + c[(path, "xy")] for c in table.values())
        y = sum(c[(path, "y")] + c[(path, "xy")] for c in table.values())
        got[path] = (x > 0, y > 0)
    return got


def warp_depth_gather(pano, lay):
    """The depth warp without a response: per tile pixel the float32 bilinear gather at
    panofuse.warp_coords' corner and weights, each operation rounded once, in the oracle's order
    (top = g00*(1-fx) + g01*fx, bot likewise, v = top*(1-fy) + bot*fy; x1 / y1 clamped)."""
    ph, pw = pano.shape
    pano = np.ascontiguousarray(pano, np.float32)
    one = np.float32(1.0)
    out = []
    for p in range(lay.ntiles):
        wxy, wf = panofuse.warp_coords(lay.fovs[p], lay.tile_w[p], lay.tile_h[p], pw, ph)
        x0 = (wxy & 0xFFFF).astype(np.int64)
        y0 = (wxy >> 16).astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, pw - 1), np.minimum(y0 + 1, ph - 1)
        fx, fy = wf[:, 0], wf[:, 1]
        top = pano[y0, x0] * (one - fx) + pano[y0, x1] * fx
        bot = pano[y1, x0] * (one - fx) + pano[y1, x1] * fx
        v = top * (one - fy) + bot * fy
        assert v.dtype == np.float32
        out.append(v)
    return np.concatenate(out)


def interleave(data1, channels=3, fill=FILL):
    """[..., n] 1-channel tile data -> [..., n * channels]: channel 0 the data, the rest fill."""
    out = np.full(data1.shape + (channels,), fill, np.float32)
    out[..., 0] = data1
    return out.reshape(data1.shape[:-1] + (-1,))


def channel(data, k, channels=3):
    return data[..., k::channels]


def fill_kept(data, channels=3, fill=FILL):
    """Do the channels past the first still hold fill?"""
    return all(bool((channel(data, k, channels) == fill).all()) for k in range(1, channels))


def oracle_warp_filled(pano, tiles, total, resp=None, fill=FILL):
    """The oracle's depth warp into a tile block prefilled with fill (pyoracle.warp_depth starts
    from zeros, which would hide a write to another channel that happens to store 0)."""
    import pyoracle as O
    ph, pw = pano.shape
    out = np.full(total, fill, np.float32)
    O.lib().pfo_warp_depth(O._p(np.ascontiguousarray(pano, np.float32)), pw, ph, tiles,
                           len(tiles), resp, O._p(out))
    return out


CHANNEL_LAYOUTS = {"MIDAS": (PL.midas_layout, (40, 30)), "LERES": (PL.leres_layout, (64, 48))}
OUT_W, EW, BATCH = 512, 128, 2
_CHANNEL_CASES = {}


def channel_case(cfg):
    """Inputs of the channel tests, built once per layout and left unchanged: the layout with
    small tiles, the oracle's tile arrays for 1 and 3 channels, per panorama a baseline and the
    warped tiles (as tests/test_gpu_layouts.py::_case builds them), 1-channel and interleaved."""
    import pf_synth
    import pyoracle as O
    if cfg in _CHANNEL_CASES:
        return _CHANNEL_CASES[cfg]
    make, size = CHANNEL_LAYOUTS[cfg]
    lay = make(*size)
    t1, n1 = O.make_tiles(lay)
    t3, n3 = O.make_tiles(lay, channels=3)
    assert n3 == 3 * n1
    emaps, gts, d1 = [], [], []
    for seed in range(BATCH):
        seeds = pf_synth.seeds_for(1, 20261020 + 101 * seed)
        emaps.append(pf_synth.baseline_emap(seeds, EW, EW // 2)[0].numpy())
        gts.append(pf_synth.scene_depth(seeds, OUT_W, OUT_W // 2)[0].numpy())
        resp = pf_synth.responses(seeds, lay.ntiles)
        d1.append(O.warp_depth(gts[-1], t1, n1, O.responses(resp)))
    d1 = np.stack(d1)
    _CHANNEL_CASES[cfg] = {"lay": lay, "t1": t1, "n1": n1, "t3": t3, "n3": n3,
                           "emaps": np.stack(emaps), "gts": np.stack(gts), "d1": d1,
                           "d3": interleave(d1)}
    return _CHANNEL_CASES[cfg]
