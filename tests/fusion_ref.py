"""The cases of tests/golden/fusion_ref.npz and the oracle's side of each of them.

TEST INFRASTRUCTURE ONLY.  tools/make_fusion_golden.py records, per case, what the compiled
reference (the unmodified Depth.cpp with the vendored Ceres 1.13, tools/fusion_ref_harness.cpp)
returns from SolveDepthToDepth, Depth2DepthTransform, SolveDepthAll, SolveDepthBySmoothing and
ErrorData; tests/test_fusion_ref.py holds the CPU oracle to the record and
tests/test_gpu_fusion_ref.py the library.  This module is what the three share: the case table,
the layouts, the decoding of the recorded inputs and the oracle calls in the reference's order.

Inputs are small on purpose: tiles hold 8-bit values (float32(u8) / float32(255)), baselines and
the ground truth 16-bit values (float32(u16) / float32(65535)).  A plane recorded whole is stored
under its name; a plane too large for the fixture is stored as <name>_sha256 plus <name>_sub, the
raveled plane at stride SUB_STRIDE.
"""
import hashlib

import numpy as np

import pf_layouts as PL
import pyoracle as O

f32 = np.float32
ZR = PL.ZENITH_RANGE
# The widest whole-degree zenith band the oracle (and the library) accept at 256 x 128: level 0
# is 64 x 32, whose band floor(32 * z0 / 180) .. ceil(32 * z1 / 180) must stay inside rows 1..30,
# so z0 >= 5.625 and z1 <= 168.75 degrees.  (3, 177) puts h1 on the last row there.
ZR_WIDE = (f32(PL.D2R(6.0)), f32(PL.D2R(168.0)))
SUB_STRIDE = 13
UNSET_BITS = 0x7FC0BEEF  # the harness's preset of median_shift_factor: ErrorData left it alone
METRIC_FIELDS = ("mse", "mae", "mre", "mselog", "delta1", "delta2", "delta3")
SETTINGS = [(a, c) for a in (0, 1, 2) for c in (0, 1)]  # align_way x cap_depth, the record's order
GT_SHAPE = (45, 90)

# name -> mode, layout, (tile_w, tile_h), tile set, (W, H), baseline, zenith range
#   merge: per-tile SolveDepthToDepth + Depth2DepthTransform, SolveDepthAll, ErrorData x 6
#   fuse: SolveDepthAll on the tiles as they are;  smooth: SolveDepthBySmoothing
CASES = {
    "c1_256x128": ("merge", "C1", (64, 64), "scene", (256, 128), "base40", ZR),
    "c1_200x100": ("merge", "C1", (64, 64), "scene", (200, 100), "base77", ZR),
    "c1_500x248": ("merge", "C1", (64, 64), "scene", (500, 248), "base40", ZR),
    "c1_384x160": ("merge", "C1", (64, 64), "scene", (384, 160), "base77", ZR),
    "leres_512x256": ("merge", "LERES", (48, 40), "leres", (512, 256), "base40d", ZR),
    "chan3_256x128": ("merge", "C1", (64, 64), "scene", (256, 128), "base77x3", ZR),
    "wide_256x128": ("merge", "WIDE", (64, 64), "wide", (256, 128), "base40", ZR_WIDE),
    "clamps_256x128": ("merge", "C1", (64, 64), "clamps", (256, 128), "base40c", ZR),
    "degenerate_256x128": ("merge", "C1", (64, 64), "degenerate", (256, 128), "base40", ZR),
    "c1_4096x256": ("fuse", "C1", (64, 64), "scene", (4096, 256), "base77", ZR),
    "smooth_256x128": ("smooth", "C1", (64, 64), "scene", (256, 128), None, ZR),
    "smooth_200x100": ("smooth", "C1", (64, 64), "scene", (200, 100), None, ZR),
    # beyond the issue's list: LERES tiles whose values span a narrow range each (see SPLIT)
    "leres_narrow_512x256": ("merge", "LERES", (48, 40), "leres_narrow", (512, 256), "base40", ZR),
}
BASELINES = {"base40": (40, 20, 1), "base77": (77, 31, 1), "base77x3": (77, 31, 3),
             "base40d": (40, 20, 1), "base40c": (40, 20, 1)}
# joint registration (SolveDepthToDepth with several active maps) on the "scene" tiles, base40
JOINT_SETS = [[0, 2], [1, 3, 4], [0, 1, 2, 3, 4, 5]]
# cases recorded whole; the others as sha256 + subsample
WHOLE = ("c1_256x128", "c1_200x100")
# the degenerate tiles of "degenerate" (tile 5 is an ordinary one)
DEGENERATE = ("constant", "two-valued", "all zero", "only 0 and 1", "half zero")
# A tile's registration is well-conditioned when the condition number of its Gauss-Newton matrix
# J'J, with the columns (x^3, x^2, x, 1) of J scaled to unit length as Ceres scales them, is at
# most KAPPA_MAX.  Two fp64 evaluations of the same LM run that differ in the order of their
# operations (Eigen's products inside Ceres, the oracle's loops, the kernel's moment sums) differ
# by a few fp64 roundings, 1.1e-16 each, which the linear solve amplifies by up to kappa; the
# coefficient is then rounded to fp32, whose half-ulp is 6e-8 relative.  At kappa <= 1e7 the
# amplified difference stays below 1e-9 * (a few), some fifty times under the half-ulp, so the
# fp32 coefficients are expected -- not guaranteed: a value may sit next to a rounding boundary --
# to be the same bits, and on every tile of the issue's cases they are; above it they are held to
# the project's stated bar instead, ABCD_RTOL (tests/test_gpu_lm.py).  The
# number is computed from the recorded inputs alone (kappa()), never from a result.
KAPPA_MAX = 1e7
ABCD_RTOL = 1e-5
# cases that hold ill-conditioned tiles: which tiles, asserted by test_golden_covers_the_cases
ILL_CONDITIONED = {"degenerate_256x128": (0, 1, 2, 3)}
# The split case: with ill-conditioned, non-degenerate tiles (kappa up to 1.4e9, coefficients up
# to 5e2 that cancel to values in 0..1) real Ceres and the oracle's two LM forms disagree in the
# last bits of a coefficient (up to 4 ulp in the record, 1 ulp on a tile of kappa 2.4e6 too), which
# moves transformed tile values by an ulp and with them some u16.  There every coefficient is
# held to ABCD_RTOL, and the transform and the fusion are pinned from the recorded coefficients
# instead of from the implementation's own.
SPLIT = ("leres_narrow_512x256",)

# Per fused case and level: (Jacobi engine, form, target patches), by the host's rules as
# tests/test_fuse_shapes.py restates them (tests/test_fusion_ref.py derives this table from them).
#   engine  "sweeps": the per-sweep kernel (a level narrower than the streamed engine's strip, or
#           a band within a row of a pole); "streamed"; "resident" (256- or 512-wide, certified)
#   form    "packed" with the separable-coverage certificate, "general" without it
#   patches "partial" where the level width is no multiple of 64
_C1_256 = (("sweeps", "packed", "full"), ("streamed", "packed", "full"),
           ("resident", "packed", "full"))
_LERES_512 = (("streamed", "packed", "full"), ("resident", "packed", "full"),
              ("resident", "packed", "full"))
ENGINES = {
    "c1_256x128": _C1_256, "chan3_256x128": _C1_256, "clamps_256x128": _C1_256,
    "degenerate_256x128": _C1_256,
    "c1_200x100": (("sweeps", "packed", "partial"), ("sweeps", "packed", "partial"),
                   ("streamed", "packed", "partial")),
    "c1_500x248": (("sweeps", "packed", "partial"), ("streamed", "packed", "partial"),
                   ("streamed", "packed", "partial")),
    "c1_384x160": (("sweeps", "packed", "partial"), ("streamed", "packed", "full"),
                   ("streamed", "packed", "full")),
    "leres_512x256": _LERES_512, "leres_narrow_512x256": _LERES_512,
    "wide_256x128": (("sweeps", "general", "full"), ("streamed", "general", "full"),
                     ("streamed", "general", "full")),
    "c1_4096x256": (("resident", "packed", "full"), ("streamed", "packed", "full"),
                    ("streamed", "packed", "full"), ("streamed", "packed", "full")),
}


def layout(name, tile):
    tw, th = tile
    if name == "C1":
        lay = PL.config_layout("C1")
    elif name == "LERES":
        lay = PL.leres_layout()
    elif name == "WIDE":  # C1's 3 x 2 windows stretched to ranges of 15..165 degrees
        lay = PL.band_layout(3, 2, tw, th, 10, 24, "wide3x2", z_lo=15.0, z_hi=165.0)
    else:
        raise ValueError(name)
    lay.tile_w[:] = tw
    lay.tile_h[:] = th
    return lay


def tiles_f32(t8):
    """float32 tiles from their uint8 record."""
    return (np.asarray(t8).astype(np.float32) / f32(255.0)).astype(np.float32)


def map_f32(m16):
    """A float32 baseline / ground truth from its uint16 record."""
    return (np.asarray(m16).astype(np.float32) / f32(65535.0)).astype(np.float32)


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def ulp_diff(a, b):
    """Per element the distance in fp32 ulps (same sign assumed where it matters)."""
    ia = bits(a).astype(np.int64)
    ib = bits(b).astype(np.int64)
    ia = np.where(ia & 0x80000000, 0x80000000 - ia, ia)
    ib = np.where(ib & 0x80000000, 0x80000000 - ib, ib)
    return np.abs(ia - ib)


def kappa(xs):
    """The condition number of the unit-column-scaled J'J of a tile's samples (see KAPPA_MAX)."""
    xs = np.asarray(xs, np.float64)
    J = np.stack([xs ** 3, xs ** 2, xs, np.ones_like(xs)], 1)
    J = J / np.linalg.norm(J, axis=0)
    return float(np.linalg.cond(J.T @ J))


def tile_kappas(tiles, data, emap, zr):
    return [kappa(O.reg_samples(tiles[p], data, emap, zr)[0]) for p in range(len(tiles))]


def abcd_mismatch(got, ref, kappas, split=False):
    """Per tile: bit equality where well-conditioned, ABCD_RTOL elsewhere (split: ABCD_RTOL on
    every tile of the case).  Returns the list of (tile, ulps, rel) that miss."""
    bad = []
    for p, k in enumerate(kappas):
        ulp = int(ulp_diff(got[p], ref[p]).max())
        rel = float(rel_diff(got[p], ref[p]).max())
        if (ulp != 0) if (k <= KAPPA_MAX and not split) else (rel > ABCD_RTOL):
            bad.append((p, ulp, rel))
    return bad


def rel_diff(got, ref):
    """The registration's stated bar (tests/test_gpu_lm.py): |got - ref| / max(|ref|, 1e-6)."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    return np.abs(got - ref) / np.maximum(np.abs(ref), 1e-6)


def record_plane(out, name, plane, whole):
    if whole:
        out[name] = plane
    else:
        out[name + "_sha256"] = sha(plane)
        out[name + "_sub"] = np.ascontiguousarray(plane).ravel()[::SUB_STRIDE].copy()


def plane_mismatch(golden, name, plane):
    """The number of recorded elements of a plane that differ (0: equal everywhere, by the whole
    plane or by its sha256)."""
    plane = np.ascontiguousarray(plane)
    if name in golden.files:
        return int((golden[name] != plane).sum())
    if np.array_equal(golden[name + "_sha256"], sha(plane)):
        return 0
    return max(1, int((golden[name + "_sub"] != plane.ravel()[::SUB_STRIDE]).sum()))


def case_inputs(golden, case):
    """(layout, oracle tiles, float32 tile data (raveled), baseline or None, (W, H), zr)."""
    mode, lname, tile, tset, size, base, zr = CASES[case]
    lay = layout(lname, tile)
    tiles, total = O.make_tiles(lay)
    data = tiles_f32(golden["tiles_" + tset]).ravel()
    assert data.size == total
    emap = map_f32(golden[base]) if base else None
    return lay, tiles, data, emap, size, zr


def oracle_levels(tiles, data, W, H, zr):
    """(oops, oob) of the oracle's targets summed over the levels of a W x H fusion."""
    oops = oob = 0
    for level in range(O.num_levels(W)):
        _, _, a, b = O.targets(tiles, data, O.level_dims(W, H, zr, level))
        oops, oob = oops + a, oob + b
    return oops, oob


def levels_double(W, H, zr):
    dims = [O.level_dims(W, H, zr, l) for l in range(O.num_levels(W))]
    return all(b.w == 2 * a.w and b.h == 2 * a.h for a, b in zip(dims, dims[1:]))


def oracle_register(tiles, data, emap, zr, form):
    """MergeDepthMaps' registration loop (Depth.cpp:794-805) on a copy of data: one tile active
    at a time, the tile transformed before the next is registered.  form: "moments" (the HIP
    kernel's form) or "samples" (Ceres' own order).  Returns (abcd float32 [n][4], data)."""
    data = data.copy()
    abcd = np.zeros((len(tiles), 4), np.float32)
    for p in range(len(tiles)):
        if form == "moments":
            _, abcd[p], deg = O.register_tile(tiles[p], data, emap, zr, solver="lm")
            assert deg == 3
        else:
            _, abcd[p], _ = O.register_tile_lm(tiles[p], data, emap, zr)
        O.depth_to_depth(tiles[p], data, abcd[p])
    return abcd, data


def joint_samples(tiles, data, emap, zr, active):
    xs, ys = [], []
    for p in active:
        x, y, _, _ = O.reg_samples(tiles[p], data, emap, zr)
        xs.append(x)
        ys.append(y)
    return np.concatenate(xs), np.concatenate(ys)


def metric_bits(d, align_way):
    """The eight recorded words of one ErrorData call from an oracle / library metrics dict."""
    v = np.array([d[k] for k in METRIC_FIELDS] + [d["median_shift"]], np.float32).view(np.uint32)
    if align_way != 1:
        v[7] = UNSET_BITS  # the reference writes median_shift_factor under align_way 1 only
    return v
