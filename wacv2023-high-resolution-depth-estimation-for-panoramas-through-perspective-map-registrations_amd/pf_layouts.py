"""Tile layouts: viewing windows (FOVs) and valid ranges, built with the reference's float32
rounding so the drop-in receives bit-identical window parameters.

* ``leres_layout`` is the active "5-fold for LeReS" table of ``Main.cpp:788-843``.
* ``midas_layout`` ("5-fold for MiDas", ``Main.cpp:731-787``), ``fold4_layout`` ("4-fold",
  ``:695-730``) and ``fold3_layout`` ("3-fold", ``:845-887``) are the reference's other tables.
* ``load_layout_file`` reads a layout file: one tile per line, eight numbers in degrees (the
  window's az_left az_right zen_top zen_down, then the range's az_left az_right zen_up zen_down),
  ``#`` comments; each value becomes ``float32(D2R(deg))``, computed in double and rounded once.
  A file with ``fold4``'s degrees is ``fold4`` bit for bit; ``leres``, ``midas`` and ``fold3`` come
  from float additions and are in general not reproduced by their rounded degrees.
* ``band_layout`` generalises the same generator pattern: azimuth sectors x
  zenith bands over [25, 155] degrees, FOV = (a_i - m, a_{i+1} + m, z_lo - zm, z_hi + zm) and range
  = (a_{i+1}, a_i, z_lo, z_hi) built exactly as ``Main.cpp:790-843`` builds them.
* ``ZENITH_RANGE`` is ``g_zenith_range`` (``Depth.cpp:22``).

Angles are radians, stored as numpy float32 arrays of shape (ntiles, 4).
"""
import math
import re
from dataclasses import dataclass

import numpy as np

MYPI = 3.14159265359  # Basic.h:11 (not exact pi)


def D2R(a):
    """Basic.h:14 -- ((a)/180.0*MYPI) in double."""
    return (a / 180.0) * MYPI


def f32(x):
    return np.float32(x)


ZENITH_RANGE = (f32(D2R(26)), f32(D2R(154)))  # Depth.cpp:22 Vec2f(D2R(26), D2R(154))
RANGE_CAP = D2R(359.9)  # Depth.cpp:783-784 MIN2(range, D2R(359.9)) (double compare)


@dataclass
class Layout:
    name: str
    fovs: np.ndarray     # (n,4) float32 {azi_left, azi_right, zen_top, zen_down}
    ranges: np.ndarray   # (n,4) float32 {azi_left, azi_right, zen_up, zen_down}, as passed in
    tile_w: np.ndarray   # (n,) int32
    tile_h: np.ndarray   # (n,) int32

    @property
    def ntiles(self):
        return int(self.fovs.shape[0])

    def capped_ranges(self):
        """The ranges MergeDepthMaps stores in each pmap (Depth.cpp:783-786)."""
        r = self.ranges.copy()
        for i in range(r.shape[0]):
            for k in (0, 1):
                v = float(r[i, k])
                r[i, k] = f32(v if v < RANGE_CAP else RANGE_CAP)
        return r


def _sector_edges(margin, a_lo_deg, a_hi_deg):
    lo = f32(D2R(a_lo_deg) - float(margin))   # float azi00 = D2R(0) - margin;
    hi = f32(D2R(a_hi_deg) + float(margin))   # float azi01 = D2R(72) + margin;
    return lo, hi


def _sector_table(name, margin_deg, nsec, fov_z, rng_z, tile_w, tile_h):
    """The generator Main.cpp's 5-fold and 3-fold tables share: nsec sectors with a margin, three
    zenith bands (degrees); tile order bands outer, sectors inner."""
    margin = f32(D2R(margin_deg))
    step = 360 // nsec
    sectors = [_sector_edges(margin, step * i, step * (i + 1)) for i in range(nsec)]
    fovs, ranges = [], []
    for (z0, z1) in fov_z:
        for (a0, a1) in sectors:
            fovs.append((a0, a1, f32(D2R(z0)), f32(D2R(z1))))
    for (z0, z1) in rng_z:
        for (a0, a1) in sectors:
            ranges.append((a1 - margin, a0 + margin, f32(D2R(z0)), f32(D2R(z1))))  # float - float
    n = len(fovs)
    return Layout(name, np.array(fovs, np.float32), np.array(ranges, np.float32),
                  np.full(n, tile_w, np.int32), np.full(n, tile_h, np.int32))


def leres_layout(tile_w=1024, tile_h=988):
    """Main.cpp:788-843 (active block): 5 sectors x 3 bands, FOV zen 18-94/52-128/86-162."""
    return _sector_table("leres5x3", 3, 5, [(18, 94), (52, 128), (86, 162)],
                         [(25, 60), (60, 120), (120, 155)], tile_w, tile_h)


def midas_layout(tile_w=1024, tile_h=727):
    """Main.cpp:731-787 ("5-fold for MiDas"): 5 sectors x 3 bands, margin 2 degrees."""
    return _sector_table("midas5x3", 2, 5, [(20, 78), (61, 119), (102, 160)],
                         [(25, 67), (67, 113), (113, 155)], tile_w, tile_h)


def fold3_layout(tile_w=1024, tile_h=749):
    """Main.cpp:845-887 ("3-fold"): 3 sectors x 3 bands, margin 2 degrees."""
    return _sector_table("fold3x3", 2, 3, [(12, 120), (36, 144), (60, 168)],
                         [(26, 60), (60, 120), (120, 154)], tile_w, tile_h)


FOLD4_DEGREES = {
    "fov_az": [(-2, 92), (88, 182), (178, 272), (268, 362)],
    "fov_zen": [(17, 109), (44, 136), (71, 163)],
    "range_az": [(90, 0), (180, 90), (270, 180), (360, 270)],
    "range_zen": [(25, 56), (56, 124), (124, 155)],
}


def fold4_layout(tile_w=1024, tile_h=989):
    """Main.cpp:695-730 ("4-fold"): every component one D2R(k) rounded to float, no arithmetic."""
    d = FOLD4_DEGREES
    fovs = [(a0, a1, z0, z1) for (z0, z1) in d["fov_zen"] for (a0, a1) in d["fov_az"]]
    ranges = [(a0, a1, z0, z1) for (z0, z1) in d["range_zen"] for (a0, a1) in d["range_az"]]
    return _degrees_layout("fold4x3", fovs, ranges, tile_w, tile_h)


def _degrees_layout(name, fovs_deg, ranges_deg, tile_w, tile_h):
    n = len(fovs_deg)
    to_rad = lambda rows: np.array([[f32(D2R(float(v))) for v in r] for r in rows], np.float32)
    return Layout(name, to_rad(fovs_deg).reshape(n, 4), to_rad(ranges_deg).reshape(n, 4),
                  np.full(n, tile_w, np.int32), np.full(n, tile_h, np.int32))


MAX_TILES = 4096  # pf_set_tiles' limit
_DECIMAL = re.compile(r"[+-]?(?:[0-9]+(?:\.[0-9]*)?|\.[0-9]+)(?:[eE][+-]?[0-9]+)?")
_FLT_MAX = float(np.finfo(np.float32).max)


def load_layout_file(path, tile_w, tile_h):
    """A layout file (module docstring), with the rules of the C++ parser (csrc/pf_layouts.cpp):
    ValueError for a line that does not hold exactly eight plain decimal numbers, a non-finite
    value, no tiles, or more than MAX_TILES tiles."""
    with open(path, "rb") as f:
        text = f.read().decode("latin-1")
    fovs, ranges = [], []
    for lineno, line in enumerate(text.split("\n"), 1):
        toks = [t for t in re.split("[ \t\r\v\f]+", line.split("#", 1)[0]) if t]
        if not toks:
            continue
        if len(toks) != 8 or not all(_DECIMAL.fullmatch(t) for t in toks):
            raise ValueError(f"{path}:{lineno}: want eight numbers (degrees)")
        if len(fovs) >= MAX_TILES:
            raise ValueError(f"{path}: more than {MAX_TILES} tiles")
        vals = [float(t) for t in toks]
        for k, v in enumerate(vals):
            if not math.isfinite(v) or not math.isfinite(D2R(v)) or abs(D2R(v)) > _FLT_MAX:
                raise ValueError(f"{path}:{lineno}: value {k + 1} is not finite")
        fovs.append(vals[:4])
        ranges.append(vals[4:])
    if not fovs:
        raise ValueError(f"{path}: no tiles")
    return _degrees_layout(f"file:{path}", fovs, ranges, tile_w, tile_h)


def tile_names(layout):
    """The <a0>_<a1>_<z0>_<z1> part of each tile's file name: round(R2D(fov)), Main.cpp:577-584
    (C round: half away from zero)."""
    def cround(x):
        return int(math.floor(abs(x) + 0.5)) * (1 if x >= 0 else -1)
    return ["_".join(str(cround(float(v) / MYPI * 180.0)) for v in f) for f in layout.fovs]


def rgb_tile_size(fov):
    """The export's tile size for a window (SaveCubeMap's viewport, Main.cpp:246-269): width 1024,
    height round(1024 / aspect) with aspect = tan(fovx/2) / tan(fovy/2) in the reference's float
    roundings."""
    fovx = f32(float(f32(fov[1]) - f32(fov[0])) / MYPI * 180.0)  # float - float
    fovy = f32(float(f32(fov[3]) - f32(fov[2])) / MYPI * 180.0)
    aspect = f32(math.tan(D2R(float(fovx)) / 2) / math.tan(D2R(float(fovy)) / 2))
    h = float(f32(1024.0) / aspect)
    return 1024, int(math.floor(h + 0.5))


def band_layout(n_az, n_bands, tile_w, tile_h, margin_deg, zmargin_deg, name=None,
                z_lo=25.0, z_hi=155.0):
    """SURVEY.md Appendix C generator (same pattern as Main.cpp:790-843)."""
    margin = f32(D2R(margin_deg))
    step = 360.0 / n_az
    sectors = [_sector_edges(margin, step * i, step * (i + 1)) for i in range(n_az)]
    zstep = (z_hi - z_lo) / n_bands
    fovs, ranges = [], []
    for j in range(n_bands):
        zl, zh = z_lo + zstep * j, z_lo + zstep * (j + 1)
        for (a0, a1) in sectors:
            fovs.append((a0, a1, f32(D2R(zl - zmargin_deg)), f32(D2R(zh + zmargin_deg))))
            ranges.append((a1 - margin, a0 + margin, f32(D2R(zl)), f32(D2R(zh))))
    n = len(fovs)
    return Layout(name or f"band{n_az}x{n_bands}", np.array(fovs, np.float32),
                  np.array(ranges, np.float32), np.full(n, tile_w, np.int32),
                  np.full(n, tile_h, np.int32))


def config_layout(cfg):
    """Layouts of BASELINE.json's configs."""
    if cfg == "C1":
        return band_layout(3, 2, 256, 256, 10, 24, "C1:3x2@256")
    if cfg in ("C2", "C3", "C4"):
        return band_layout(5, 4, 512, 512, 3, 12, "C2:5x4@512")
    if cfg == "C5":
        return band_layout(10, 8, 1024, 1024, 3, 8, "C5:10x8@1024")
    if cfg == "LERES":
        return leres_layout()
    if cfg == "MIDAS":
        return midas_layout()
    if cfg == "FOLD4":
        return fold4_layout()
    if cfg == "FOLD3":
        return fold3_layout()
    raise ValueError(cfg)


CONFIGS = {
    # name: (out_w, emap_w, layout)
    "C1": (512, 128),
    "C2": (2048, 512),
    "C5": (8192, 2048),
}
