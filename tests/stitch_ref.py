"""CPU restatement of the direct tile stitch (csrc/pf_stitch.hip: MergeDepthMaps' `if (false)`
block, Depth.cpp:817-865) and of SolveDepthAll's Laplacian self-check (Depth.cpp:1738-1758).

TEST INFRASTRUCTURE ONLY.  Every fp32 expression of the reference is one numpy float32 operation
per rounding, in the reference's operand order; the azimuth / zenith of a pixel are the fusion
grid's (float32 of a double product with MYPI) and their sines and cosines come from glibc's
sincosf, which is what the reference's g++ build calls.  The tiles' cached windows (middle,
hedge, vedge, corner0: PerspectiveMap::SetWindow) and their ranges are taken from the oracle's
tile records (oracle/pyoracle.py make_tiles); tests/golden/stitch_ref.npz pins the whole chain
to the reference's own SetWindow / SphericalTo2D / Value / Depth2DepthTransform.
"""
import ctypes as C
import math

import numpy as np

MYPI = 3.14159265359  # Basic.h:11
NAN_MARKER = 0x7FBADBAD  # the library's un-windowed marker in a target plane
f32 = np.float32

_libm = C.CDLL("libm.so.6")
_libm.sincosf.argtypes = [C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float)]
_libm.sincosf.restype = None


GOLDEN_TILE = 64  # tests/golden/stitch_ref.npz: the C1 windows with 64 x 64 tiles


def golden_layout():
    """The layout of tests/golden/stitch_ref.npz (tools/make_stitch_golden.py)."""
    import pf_layouts as PL
    lay = PL.config_layout("C1")
    lay.tile_w[:] = GOLDEN_TILE
    lay.tile_h[:] = GOLDEN_TILE
    return lay


def golden_tiles(t8):
    """The golden's float tiles [ntiles][64][64] from its uint8 record."""
    return (np.asarray(t8).astype(np.float32) / f32(255.0)).astype(np.float32)


def _sincosf(vals):
    s = np.zeros(len(vals), np.float32)
    c = np.zeros(len(vals), np.float32)
    a, b = C.c_float(), C.c_float()
    for i, v in enumerate(vals):
        _libm.sincosf(float(v), C.byref(a), C.byref(b))
        s[i], c[i] = a.value, b.value
    return s, c


def c_round(v):
    """C round(): to nearest, halves away from zero."""
    a = abs(v)
    r = math.floor(a)
    if a - r >= 0.5:
        r += 1
    return int(r) if v >= 0 else -int(r)


def grid(W, H):
    """(az [W], zen [H]) float32 of the output pixels (Depth.cpp:827)."""
    X = np.arange(W, dtype=np.float32)
    Y = np.arange(H, dtype=np.float32)
    az = ((X / f32(W - 1) * f32(2)).astype(np.float64) * MYPI).astype(np.float32)
    zen = ((Y / f32(H - 1)).astype(np.float64) * MYPI).astype(np.float32)
    return az, zen


def boxes(tiles, W, H):
    """Per tile (x0, x1, y0, y1) (Depth.cpp:834-837): doubles, C round."""
    out = []
    for t in tiles:
        r = [float(t.ranges[k]) for k in range(4)]
        out.append((c_round(r[0] / (2 * MYPI) * (W - 1)), c_round(r[1] / (2 * MYPI) * (W - 1)),
                    c_round(r[2] / MYPI * (H - 1)), c_round(r[3] / MYPI * (H - 1))))
    return out


def cover(tiles, W, H):
    """count [H][W]: the number of tile boxes holding each pixel; first [H][W]: the first tile
    (ascending order) whose box holds it, -1 under no tile.  Both box ends are inclusive."""
    first = np.full((H, W), -1, np.int32)
    count = np.zeros((H, W), np.int32)
    X = np.arange(W)[None, :]
    Y = np.arange(H)[:, None]
    for p, (x0, x1, y0, y1) in enumerate(boxes(tiles, W, H)):
        inside = (X >= min(x0, x1)) & (X <= max(x0, x1)) & (Y >= y0) & (Y <= y1)
        first[inside & (first < 0)] = p
        count += inside
    return count, first


def _v3(a):
    return [f32(a[0]), f32(a[1]), f32(a[2])]


def _dot(a, b):
    return f32(f32(f32(a[0] * b[0]) + f32(a[1] * b[1])) + f32(a[2] * b[2]))


def tile_indices(t, W, H):
    """Per output pixel the linear element index (Y * w + X) * channels of Value(SphericalTo2D(az,
    zen)) in tile record t, int64 [H][W], unclamped (Depth.cpp:168-182, 111-118, 34-42)."""
    az, zen = grid(W, H)
    sa, ca = _sincosf(az)
    sz, cz = _sincosf(zen)
    mid, hed, ved, c0 = _v3(t.middle), _v3(t.hedge), _v3(t.vedge), _v3(t.corner0)
    mm = _dot([f32(m - f32(0)) for m in mid], mid)
    hl = f32(np.sqrt(_dot(hed, hed)))
    vl = f32(np.sqrt(_dot(ved, ved)))
    with np.errstate(all="ignore"):
        d0 = sz[:, None] * ca[None, :]  # SphericalToWorld (Depth.cpp:2955-2958)
        d1 = sz[:, None] * sa[None, :]
        d2 = np.broadcast_to(cz[:, None], d0.shape)
        den = (d0 * mid[0] + d1 * mid[1]) + d2 * mid[2]
        tt = mm / den
        e = [(f32(0) + tt * d) - c for d, c in zip((d0, d1, d2), c0)]
        eh = (e[0] * hed[0] + e[1] * hed[1]) + e[2] * hed[2]
        ev = (e[0] * ved[0] + e[1] * ved[1]) + e[2] * ved[2]
        x = (eh / hl) / hl
        y = (ev / vl) / vl
        # int X = x * (float)(width - 1): truncation toward zero
        Xi = np.trunc(x * f32(t.width - 1)).astype(np.int64)
        Yi = np.trunc(y * f32(t.height - 1)).astype(np.int64)
    return (Yi * t.width + Xi) * t.channels


def cubic_map(X, abcd):
    """Depth2DepthTransform's per-value map (Depth.cpp:256-271) of a float32 array in fp32."""
    a, b, c, d = [f32(v) for v in np.asarray(abcd, np.float32)]
    X = np.asarray(X, np.float32).copy()
    wide = X.astype(np.float64)
    lo = wide < 1e-4
    hi = ~lo & (wide > (1 - 1e-4))
    X[lo] = f32(1e-4)
    X[hi] = f32(1 - 1e-4)
    with np.errstate(all="ignore"):
        Y = (((a * X * X * X + b * X * X) + c * X) + d).astype(np.float32)
    neg = Y < 0
    big = ~neg & (Y > 1)
    Y[neg] = f32(0)
    Y[big] = f32(1)
    return Y


def quantize(v):
    """The library's quantiser: clamp to [0, 1], (u16)(v * 65535.0f), NaN -> 0."""
    v = np.asarray(v, np.float32).copy()
    nan = np.isnan(v)
    v[nan] = 0
    v = np.minimum(np.maximum(v, f32(0)), f32(1))
    return (v * f32(65535.0)).astype(np.float32).astype(np.uint16)


def stitch(tiles, tile_data, W, H, coeffs=None, stats=None):
    """The direct stitch of one panorama: uint16 [H][W].  tiles: the oracle's tile records;
    tile_data: float32 [tile_elems]; coeffs: None or [ntiles][4].  stats (a dict, optional)
    receives `outside`: the number of pixels whose index left its tile (clamped here as the
    library clamps it; the reference reads out of bounds there)."""
    tile_data = np.asarray(tile_data, np.float32).ravel()
    _, first = cover(tiles, W, H)
    out = np.zeros((H, W), np.uint16)
    outside = 0
    for p, t in enumerate(tiles):
        sel = first == p
        if not sel.any():
            continue
        idx = tile_indices(t, W, H)[sel]
        lim = t.width * t.height * t.channels
        outside += int(((idx < 0) | (idx >= lim)).sum())
        idx = np.where(idx < 0, 0, idx)
        idx = np.where(idx >= lim, lim - t.channels, idx)
        v = tile_data[t.offset + idx]
        if coeffs is not None:
            v = cubic_map(v, coeffs[p])
        out[sel] = quantize(v)
    if stats is not None:
        stats["outside"] = outside
    return out


def sq_step(acc, d):
    """err += pow(d, 2) on a float err (Depth.cpp:1754): the exact double square, one rounding."""
    t = float(d)
    return f32(float(acc) + t * t)


def laplacian_terms(buf, lnorm, h0, h1):
    """d = Laplacian_cur - target (fp32) for rows h0+1 .. h1-1, columns 1 .. w-2, row-major.  A
    target that carries the un-windowed marker counts as 0 (Depth.h:268-271)."""
    b = np.asarray(buf, np.float32)
    bits = np.ascontiguousarray(lnorm, np.float32).view(np.uint32)
    L = np.where(bits == NAN_MARKER, f32(0), np.asarray(lnorm, np.float32)).astype(np.float32)
    ys = slice(h0 + 1, h1)
    with np.errstate(all="ignore"):
        val = b[ys, 1:-1]
        s = ((b[ys, :-2] + b[ys, 2:]) + b[h0:h1 - 1, 1:-1]) + b[h0 + 2:h1 + 1, 1:-1]
        cur = val - s / f32(4)
        return (cur - L[ys, 1:-1]).astype(np.float32).ravel()


def laplacian_residual(buf, lnorm, h0, h1):
    """The reference's float chain over one plane: float32."""
    h, w = np.asarray(buf).shape
    if not (0 <= h0 and h0 + 2 <= h1 <= h - 1 and w >= 3):
        raise ValueError("rows / width out of range")
    acc = 0.0  # a float32 value held in a Python float: (float)((double)err + d*d) per step
    for d in laplacian_terms(buf, lnorm, h0, h1).astype(np.float64):
        acc = float(f32(acc + d * d))
    return f32(acc)
