"""fp64 numpy restatement of DepthNamespace::ErrorLaplacian (Depth.cpp:2636-2953); a helper of
tests/test_edge_ref.py, tests/test_gpu_edge*.py and tools/make_edge_golden.py, not a test.

gt, given: 2-D float32 arrays (channel 0 of the maps).  Per given pixel (x, y) the gt taps sit
at X = (int)((float)x * ratio_x) with ratio_x = (float)gw / (float)w in fp32 (Depth.cpp:2654-2655,
:2692-2697); every tap is widened to double and the filters are evaluated in fp64 in the
reference's left-to-right order; the sums are math.fsum (exact, then rounded once)."""
import math

import numpy as np

KEYS = ("lap_mse", "lap_mae", "sobelx_mae", "sobely_mae", "lap5_mae")
COUNTS = ("n_lap", "n_sobel", "n_lap5")


def u16_to_float(a):
    """EquirectangularMap::Load of a 16-bit image: (float)v / 65535.0f (Depth.cpp:322)."""
    return (np.asarray(a).astype(np.float32) / np.float32(65535.0)).astype(np.float32)


def write_png16(path, a):
    """A 16-bit gray PNG of the u16 array a [h][w] (zlib only)."""
    import struct
    import zlib
    a = np.ascontiguousarray(a, np.uint16)
    h, w = a.shape
    raw = b"".join(b"\x00" + a[y].astype(">u2").tobytes() for y in range(h))

    def chunk(tag, data):
        body = tag + data
        return struct.pack(">I", len(data)) + body + struct.pack(">I", zlib.crc32(body))
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 16, 0, 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def read_png16(path):
    """The u16 array [h][w] of a 16-bit gray, non-interlaced PNG whose rows use filter 0 (what
    this project's writer and write_png16 produce)."""
    import struct
    import zlib
    d = open(path, "rb").read()
    pos, idat = 8, b""
    while pos < len(d):
        n = struct.unpack(">I", d[pos:pos + 4])[0]
        tag, body = d[pos + 4:pos + 8], d[pos + 8:pos + 8 + n]
        if tag == b"IHDR":
            w, h, depth, ctype = struct.unpack(">IIBB", body[:10])
            assert (depth, ctype) == (16, 0)
        elif tag == b"IDAT":
            idat += body
        pos += 12 + n
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 2 * w + 1)
    assert not rows[:, 0].any()
    return np.ascontiguousarray(rows[:, 1:]).view(">u2").astype(np.uint16)


def tap_index(n_given, n_gt):
    """(int)((float)i * ((float)n_gt / (float)n_given)) for i = 0 .. n_given - 1."""
    ratio = np.float32(n_gt) / np.float32(n_given)
    return (np.arange(n_given, dtype=np.float32) * ratio).astype(np.int64)


def _window(img, iy, ix, ys, xs, di, dj):
    """img[iy[y + dj], ix[x + di]] over the sample grid ys x xs, as float64."""
    return img[np.ix_(iy[ys + dj], ix[xs + di])].astype(np.float64)


def edge_terms(gt, given, strict_sobel=False):
    """Per-sample terms and maps.  strict_sobel tests all nine taps instead of the reference's
    list (Depth.cpp:2747-2748), for the test that shows the two differ."""
    gt = np.asarray(gt, np.float32)
    given = np.asarray(given, np.float32)
    gh, gw = gt.shape
    h, w = given.shape
    ix, iy = tap_index(w, gw), tap_index(h, gh)
    jx, jy = np.arange(w), np.arange(h)
    maps = {k: np.zeros((h, w), np.float64) for k in ("gt_lap", "given_lap", "lap_ae")}
    empty = np.zeros(0, np.float64)
    out = {"lap_sq": empty, "lap_abs": empty, "sobelx": empty, "sobely": empty, "lap5": empty,
           "maps": maps}

    if w >= 3 and h >= 3:
        xs, ys = np.arange(1, w - 1), np.arange(1, h - 1)
        # the range test of Depth.cpp:2698
        okx = (ix[xs - 1] >= 0) & (ix[xs + 1] <= gw - 1)
        oky = (iy[ys - 1] >= 0) & (iy[ys + 1] <= gh - 1)
        xs, ys = xs[okx], ys[oky]
        # val[a][b] of the reference = V[(a - 1, b - 1)] (a: x offset, b: y offset)
        V = {(di, dj): _window(gt, iy, ix, ys, xs, di, dj) for di in (-1, 0, 1) for dj in (-1, 0, 1)}
        B = {(di, dj): _window(given, jy, jx, ys, xs, di, dj) for di in (-1, 0, 1) for dj in (-1, 0, 1)}
        val = lambda a, b: V[(a - 1, b - 1)]  # noqa: E731
        Val = lambda a, b: B[(a - 1, b - 1)]  # noqa: E731
        bad = ((val(1, 1) < 1e-4) | (val(0, 1) < 1e-4) | (val(2, 1) < 1e-4) | (val(1, 0) < 1e-4) |
               (val(1, 2) < 1e-4))
        gl = 1 * val(1, 1) - (val(0, 1) + val(2, 1) + val(1, 0) + val(1, 2)) / 4
        bl = 1 * Val(1, 1) - (Val(0, 1) + Val(2, 1) + Val(1, 0) + Val(1, 2)) / 4
        ok = ~bad
        d = gl - bl
        out["lap_sq"] = (d * d)[ok]
        out["lap_abs"] = np.abs(d)[ok]
        sub = np.ix_(ys, xs)
        maps["gt_lap"][sub] = np.where(ok, gl, 0.0)
        maps["given_lap"][sub] = np.where(ok, bl, 0.0)
        maps["lap_ae"][sub] = np.where(ok, np.abs(d), 0.0)
        # the reference's list as written: [0][1] and [0][2] twice, [1][0] and [2][0] never
        taps = [(0, 0), (0, 1), (0, 2), (0, 1), (1, 1), (2, 1), (0, 2), (1, 2), (2, 2)]
        if strict_sobel:
            taps = [(a, b) for a in range(3) for b in range(3)]
        sbad = np.zeros_like(bad)
        for a, b in taps:
            sbad |= val(a, b) < 1e-4
        gsx = val(0, 0) - val(2, 0) + 2 * val(0, 1) - 2 * val(2, 1) + val(0, 2) - val(2, 2)
        gsy = val(0, 0) + 2 * val(1, 0) + val(2, 0) - val(0, 2) - 2 * val(1, 2) - val(2, 2)
        bsx = Val(0, 0) - Val(2, 0) + 2 * Val(0, 1) - 2 * Val(2, 1) + Val(0, 2) - Val(2, 2)
        bsy = Val(0, 0) + 2 * Val(1, 0) + Val(2, 0) - Val(0, 2) - 2 * Val(1, 2) - Val(2, 2)
        out["sobelx"] = np.abs(gsx - bsx)[~sbad]
        out["sobely"] = np.abs(gsy - bsy)[~sbad]

    if w >= 5 and h >= 5:
        xs, ys = np.arange(2, w - 2), np.arange(2, h - 2)
        # Depth.cpp:2856-2857 tests X0 and X2 only; X4 is bounded too (never true at the sizes the
        # tests use: a sample would be skipped, not read out of range)
        okx = (ix[xs - 2] >= 0) & (ix[xs] <= gw - 1) & (ix[xs + 2] <= gw - 1)
        oky = (iy[ys - 2] >= 0) & (iy[ys] <= gh - 1) & (iy[ys + 2] <= gh - 1)
        xs, ys = xs[okx], ys[oky]
        rng = (-2, -1, 0, 1, 2)
        V = {(di, dj): _window(gt, iy, ix, ys, xs, di, dj) for di in rng for dj in rng}
        B = {(di, dj): _window(given, jy, jx, ys, xs, di, dj) for di in rng for dj in rng
             if abs(di) + abs(dj) <= 2}  # the 13 taps of the LoG filter
        bad = np.zeros(V[(0, 0)].shape, bool)
        for k in V:
            bad |= V[k] < 1e-4

        def log5(T):
            v = lambda a, b: T[(a - 2, b - 2)]  # noqa: E731
            return (-1 * v(2, 0) - 1 * v(1, 1) - 2 * v(2, 1) - 1 * v(3, 1)
                    - 1 * v(0, 2) - 2 * v(1, 2) + 16 * v(2, 2) - 2 * v(3, 2) - 1 * v(4, 2)
                    - 1 * v(1, 3) - 2 * v(2, 3) - 1 * v(3, 3) - 1 * v(2, 4))
        out["lap5"] = np.abs(log5(V) - log5(B))[~bad]
    return out


def _mean(terms):
    n = int(terms.size)
    return (math.fsum(terms.tolist()) / n) if n else float("nan")


def edge_metrics(gt, given, strict_sobel=False, maps=False):
    """The five means (exact sums, one rounding, one divide) and the three counts."""
    t = edge_terms(gt, given, strict_sobel)
    r = {"lap_mse": _mean(t["lap_sq"]), "lap_mae": _mean(t["lap_abs"]),
         "sobelx_mae": _mean(t["sobelx"]), "sobely_mae": _mean(t["sobely"]),
         "lap5_mae": _mean(t["lap5"]),
         "n_lap": int(t["lap_sq"].size), "n_sobel": int(t["sobelx"].size),
         "n_lap5": int(t["lap5"].size)}
    return (r, t["maps"]) if maps else r


def mean_bound(w, h):
    """|got - exact| <= 2 * N * 2^-53 * exact, N = w * h: any order of N non-negative fp64 terms
    is within (N - 1) * 2^-53 relative of the exact sum; the factor 2 covers the divide."""
    return 2.0 * w * h * 2.0 ** -53


def close(got, exact, w, h):
    if math.isnan(exact):
        return math.isnan(got)
    return abs(got - exact) <= mean_bound(w, h) * abs(exact)
