"""Inputs that tests/test_disp_weight_ref.py and tests/test_gpu_disp_weights.py share: the synthetic
C1 disparity tiles of tests/test_gpu_disp.py (per-tile normalised inverse depth of the warped
scene), the one-tile 121 x 121 grid above the resident capacity, and the weight fields.

TEST INFRASTRUCTURE ONLY.  Everything is cached per process and read-only.
"""
import functools

import numpy as np

import pf_layouts as PL
import pf_synth
import pyoracle as O

f32 = np.float32
ZR = PL.ZENITH_RANGE
EW = 128


def to_disparity(data, tiles):
    """MiDaS' convention per tile: (1 / max(t, 0.02) - min) / (max - min)."""
    out = np.empty_like(data)
    for t in tiles:
        n = t.width * t.height * t.channels
        inv = f32(1.0) / np.maximum(data[t.offset:t.offset + n], f32(0.02))
        lo, hi = inv.min(), inv.max()
        out[t.offset:t.offset + n] = (inv - lo) / (hi - lo)
    return out


def inputs(lay, seed, out_w=512):
    """(oracle tiles, emap [64][128], disparity tile data) of one synthetic panorama."""
    tiles, total = O.make_tiles(lay)
    seeds = pf_synth.seeds_for(1, 20261015 + 1000 * seed)
    emap = pf_synth.baseline_emap(seeds, EW, EW // 2)[0].numpy()
    gt = pf_synth.scene_depth(seeds, out_w, out_w // 2)[0].numpy()
    depth = O.warp_depth(gt, tiles, total, O.responses(pf_synth.responses(seeds, lay.ntiles)))
    disp = to_disparity(depth, tiles)
    emap.setflags(write=False)
    disp.setflags(write=False)
    return tiles, emap, disp


@functools.lru_cache(maxsize=None)
def c1(seed):
    """(layout, tiles, emap, disp) of C1: 6 tiles of 256^2, 7,865 samples each."""
    lay = PL.config_layout("C1")
    return (lay,) + inputs(lay, seed)


@functools.lru_cache(maxsize=None)
def wide():
    """One 256^2 tile with 121 x 121 = 14,641 samples: above the resident capacity of 8,192."""
    full = PL.band_layout(3, 1, 256, 256, 10, 10, z_lo=30.0, z_hi=150.0)
    lay = PL.Layout("one-wide-tile", full.fovs[:1].copy(), full.ranges[:1].copy(),
                    full.tile_w[:1].copy(), full.tile_h[:1].copy())
    return (lay,) + inputs(lay, 4)


def smooth_field(tiles, seed):
    """A fixed-seed weight set: per tile an 8 x 8 grid of values in [0.1, 1] upsampled bilinearly,
    in channel 0 (the field of tests/test_gpu_weights.py); the other channels hold junk."""
    rs = np.random.RandomState(seed)
    total = sum(t.width * t.height * t.channels for t in tiles)
    out = rs.rand(total).astype(f32) * f32(3) - f32(1.5)
    for t in tiles:
        w, h, c = t.width, t.height, t.channels
        g = (0.1 + 0.9 * rs.rand(8, 8)).astype(np.float64)
        ys = np.linspace(0, 7, h)
        xs = np.linspace(0, 7, w)
        y0 = np.minimum(ys.astype(int), 6)
        x0 = np.minimum(xs.astype(int), 6)
        fy = (ys - y0)[:, None]
        fx = (xs - x0)[None, :]
        v = ((1 - fy) * (1 - fx) * g[y0][:, x0] + (1 - fy) * fx * g[y0][:, x0 + 1]
             + fy * (1 - fx) * g[y0 + 1][:, x0] + fy * fx * g[y0 + 1][:, x0 + 1])
        out[t.offset:t.offset + w * h * c:c] = v.astype(f32).reshape(-1)
    return out


def zero_rect(tiles, weights, p=0):
    """`weights` with an exact-zero rectangle in tile p: rows 39 % .. 100 %, columns 39 % .. 70 %."""
    w = np.array(weights, f32)
    t = tiles[p]
    v = w[t.offset:t.offset + t.width * t.height * t.channels].reshape(t.height, t.width,
                                                                       t.channels)
    v[int(t.height * 100 / 256):, int(t.width * 100 / 256):int(t.width * 180 / 256), 0] = 0.0
    return w


@functools.lru_cache(maxsize=None)
def c1_field():
    w = zero_rect(c1(0)[1], smooth_field(c1(0)[1], 20261021))
    w.setflags(write=False)
    return w


def sky(tiles, disp, rows=96):
    """The tiles with their top `rows` rows set to disparity 0: what a network writes for sky."""
    d = np.array(disp, f32)
    for t in tiles:
        v = d[t.offset:t.offset + t.width * t.height * t.channels].reshape(t.height, t.width,
                                                                           t.channels)
        v[:rows, :, 0] = 0.0
    return d
