"""Restatement of DepthNamespace::ErrorCompare (Depth.cpp:2460-2634) with the pieces it is built
on, EquirectangularMap::DispDepthConversion and Save8bit (Depth.cpp:587-635); a helper of
tests/test_compare_ref.py, tests/test_gpu_compare*.py and tools/make_compare_golden.py, not a
test.  Both ErrorEmap calls go through the CPU oracle (pyoracle.error_metrics); everything else is
numpy float32, one rounding per operation.

The chain, on channel 0 of the maps:
  depth mode      metrics = ErrorEmap(gt, given, align_way, cap); shifted = quantise(given).
  disparity mode  gt_disp = conv(gt, gc); {s, o} = ErrorEmap(gt_disp, given, 2, no cap);
                  v = given * s + o; v = conv(v, given_c); v < 0 -> 0, v > 10 -> 10 (the depth
                  plane); metrics = ErrorEmap(gt, v, align_way, cap); vmin / vmax over the pixels
                  with (double)|v| >= 1e-4, which become (v - vmin) / (vmax - vmin); quantise.
conv(a, C) inverts a value with (double)|v| >= 1e-5 and keeps any other, C times over: the
reference loops over the C channels but reads and writes channel 0 each time.

Where the reference's behaviour is undefined the project's rule holds: a product above 255
saturates to 255 and NaN becomes 0 in the u8 plane; every comparison follows IEEE, so a NaN is
not black, does not move vmin / vmax and stays NaN in the depth plane."""
import struct
import zlib

import numpy as np

import pyoracle as O

F32 = np.float32
FLT_MAX = float(np.finfo(np.float32).max)
METRICS = ("mse", "mae", "mre", "mselog", "delta1", "delta2", "delta3")
# file kinds of the golden inputs: how an array becomes a file and a loaded map
KINDS = ("png16", "png8", "pfm")


def conv(v, times):
    """DispDepthConversion of channel 0 of a map with `times` channels (Depth.cpp:587-610)."""
    v = np.array(v, F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        for _ in range(int(times)):
            small = np.abs(v).astype(np.float64) < 1e-5
            v = np.where(small, v, F32(1.0) / np.where(small, F32(1.0), v)).astype(F32)
    return v


def quantise(v):
    """(unsigned char)(max(v, 0) * 255.0f) with the saturation and NaN rules."""
    v = np.array(v, F32)
    with np.errstate(invalid="ignore"):
        v = np.where(v < 0, F32(0.0), v)
        p = (v * F32(255.0)).astype(F32)
        q = np.where(p >= F32(255.0), F32(255.0), p)
    q = np.where(np.isnan(q), F32(0.0), q)
    return np.trunc(q).astype(np.uint8)


def save8bit(v):
    """The u8 plane of EquirectangularMap::Save8bit (Depth.cpp:612-635): clamp to 0..1 first."""
    v = np.array(v, F32)
    with np.errstate(invalid="ignore"):
        v = np.where(v < 0, F32(0.0), v)
        v = np.where(v > 1, F32(1.0), v)
    return quantise(v)


def _ch0(a):
    a = np.asarray(a, F32)
    return a[..., 0] if a.ndim == 3 else a


def _channels(a):
    return a.shape[2] if a.ndim == 3 else 1


def _with_ch0(a, v):
    a = np.array(a, F32)
    if a.ndim == 3:
        a[..., 0] = v
    else:
        a[...] = v
    return a


def minmax_nonblack(v):
    """(vmin, vmax, nonblack mask) of Depth.cpp:2537-2551: from FLT_MAX / -FLT_MAX over the pixels
    that are not black; a NaN is not black and moves neither."""
    nonblack = ~(np.abs(v).astype(np.float64) < 1e-4)
    vals = v[nonblack & ~np.isnan(v)]
    vmin = F32(min(FLT_MAX, float(vals.min()))) if vals.size else F32(FLT_MAX)
    vmax = F32(max(-FLT_MAX, float(vals.max()))) if vals.size else F32(-FLT_MAX)
    return vmin, vmax, nonblack


def depth_plane(given, given_c, s, o):
    """Steps 3-5 of the disparity chain for a known fit."""
    v = (_ch0(given) * F32(s)).astype(F32)
    v = (v + F32(o)).astype(F32)
    v = conv(v, given_c)
    with np.errstate(invalid="ignore"):
        v = np.where(v < 0, F32(0.0), v)
        v = np.where(v > 10, F32(10.0), v)
    return v.astype(F32)


def normalise(v):
    """Steps 7-8: (vmin, vmax, n_nonblack, normalised plane)."""
    vmin, vmax, nonblack = minmax_nonblack(v)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        nv = ((v - vmin).astype(F32) / (vmax - vmin).astype(F32)).astype(F32)
    return vmin, vmax, int(nonblack.sum()), np.where(nonblack, nv, v).astype(F32)


def compare(gt, given, zr, disp_depth, align_way, cap_depth, fit=None):
    """ErrorCompare on two loaded maps (float32 [h][w] or [h][w][c]).  Returns a dict: the final
    ErrorEmap's fields (pyoracle.METRIC_KEYS, n, nlog), fit_s, fit_o, vmin, vmax, n_nonblack,
    'depth' (float32 [h][w]: the map the final ErrorEmap scored) and 'shifted' (uint8 [h][w]).
    fit: use this {s, o} instead of the oracle's least-squares fit."""
    gt = np.asarray(gt, F32)
    given = np.asarray(given, F32)
    if not disp_depth:
        r = dict(O.error_metrics(gt, given, zr, align_way, cap_depth))
        r.update(fit_s=0.0, fit_o=0.0, vmin=FLT_MAX, vmax=-FLT_MAX, n_nonblack=0,
                 depth=_ch0(given).copy(), shifted=quantise(_ch0(given)))
        return r
    if fit is None:
        gt_disp = _with_ch0(gt, conv(_ch0(gt), _channels(gt)))
        f = O.error_metrics(gt_disp, given, zr, 2, False)
        fit = (f["ls_s"], f["ls_o"])
    s, o = F32(fit[0]), F32(fit[1])
    v = depth_plane(given, _channels(given), s, o)
    r = dict(O.error_metrics(gt, _with_ch0(given, v), zr, align_way, cap_depth))
    vmin, vmax, n, nv = normalise(v)
    r.update(fit_s=float(s), fit_o=float(o), vmin=float(vmin), vmax=float(vmax), n_nonblack=n,
             depth=v, shifted=quantise(nv))
    return r


# ---- the golden inputs as files and as loaded maps ----
def load_map(a, kind, mono360=False):
    """EquirectangularMap::Load (Depth.cpp:277-355, LoadPfm :455-549) of the file that write_file
    makes of array a: u16 / 65535.0f, u8 / 255.0f; a PFM keeps its file's bottom-up rows, which
    mono360 flips and normalises to 0..1 (else the value is max(v, 0) / 10 capped at 10)."""
    a = np.asarray(a)
    if kind == "png16":
        return (a.astype(F32) / F32(65535.0)).astype(F32)
    if kind == "png8":
        return (a.astype(F32) / F32(255.0)).astype(F32)
    assert kind == "pfm"
    a = a.astype(F32)
    if mono360:
        lo, hi = F32(a.min()), F32(a.max())
        return ((a[::-1] - lo).astype(F32) / F32(hi - lo)).astype(F32)
    return np.minimum((np.maximum(a, F32(0.0)) / F32(10.0)).astype(F32), F32(10.0))


def _chunk(tag, data):
    body = tag + data
    return struct.pack(">I", len(data)) + body + struct.pack(">I", zlib.crc32(body))


def write_file(path, a, kind):
    """a as a file of the given kind at path (the extension must fit: .png or .pfm).  png16:
    u16 [h][w] gray; png8: u8 [h][w] gray or [h][w][c], c = 2 gray+alpha, 3 RGB, 4 RGBA; pfm:
    float32 [h][w], little-endian "Pf", rows in the array's order."""
    a = np.ascontiguousarray(a)
    if kind == "pfm":
        h, w = a.shape
        with open(path, "wb") as f:
            f.write(b"Pf\n%d %d\n-1.0\n" % (w, h) + a.astype("<f4").tobytes())
        return
    h, w = a.shape[:2]
    c = a.shape[2] if a.ndim == 3 else 1
    depth = 16 if kind == "png16" else 8
    ctype = {1: 0, 2: 4, 3: 2, 4: 6}[c]
    rows = a.reshape(h, w * c).astype(">u2" if depth == 16 else np.uint8)
    raw = b"".join(b"\x00" + rows[y].tobytes() for y in range(h))
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, 0))
                + _chunk(b"IDAT", zlib.compress(raw, 9)) + _chunk(b"IEND", b""))


def extension(kind):
    return ".pfm" if kind == "pfm" else ".png"


def golden_cases(z):
    """The runs of tests/golden/compare_ref.npz: dicts with the two raw arrays and their kinds,
    the flags, the reference's seven float32, its shifted pixels and its PNG file's bytes."""
    names = [str(n) for n in z["array_names"]]
    kinds = [KINDS[k] for k in z["array_kinds"]]
    runs = []
    for i, (pair, disp, align, cap) in enumerate(z["runs"].tolist()):
        ig, iv = z["pairs"][pair].tolist()
        plane = int(z["plane_of"][pair][disp])
        runs.append({"id": f"pair{pair}-{'disp' if disp else 'depth'}-a{align}-{'cap' if cap else 'nocap'}",
                     "pair": pair, "gt_raw": z[names[ig]], "gt_kind": kinds[ig],
                     "given_raw": z[names[iv]], "given_kind": kinds[iv],
                     "disp": bool(disp), "align_way": int(align), "cap": bool(cap),
                     "ref": z["ref"][i].astype(F32),
                     "pixels": z[f"pixels{plane}"], "png": z[f"png{plane}"].tobytes()})
    return runs
