"""CPU restatement of the overlap-consistent registration (csrc/pf_consist.hip).

TEST INFRASTRUCTURE ONLY.  Per panorama, with c_p the cubic of tile p,

  E(c) = sum_p sum_{s in S_p} (u_s.c_p - y_s)^2 + lam sum_{(p,q)} sum_{s in O_pq} (u_s.c_p - v_s.c_q)^2

S_p the registration samples of tile p, O_pq those of them whose grid direction falls inside tile
q's window, u = (X^3, X^2, X, 1) of tile p's clamped value and v the same row of tile q's.
Everything below follows the kernels operation for operation in IEEE-754 fp64 + - * / sqrt, so the
two agree bit for bit:

  data_sums / pair_sums   k_register's 15 sums and k_pair_moments' 36, in the lane order and tree of
                          planar_ref.ordered_sums (lane l of 256 adds samples l, l + 256, ... from
                          0.0, then the halving tree)
  assemble                the normal equations A c = r (lower triangle): diagonal block p is M_p,
                          then + lam U_pq in ascending q, then + lam V_qp in ascending q; block
                          (a, b), a > b, is -(lam (C_ab + C_ba')) with a missing pair as 0.0
  cholesky_solve          right-looking in-place Cholesky (an outer-product update is one multiply
                          and one subtract per element, as in the kernel) and the two
                          column-oriented substitutions; None where a pivot is not > 0 or the
                          solution is not finite
  costs                   the two terms of E from the moment sums (mom_cost's loop order)
  register                all of it for one panorama: (coeffs64 [ntiles][4], summary [4])
  overlap_stats           k_overlap_stats: {count, sum d, sum d^2, max |d|, NaN samples} per pair

The pair table itself is the device's in the GPU tests.  pair_table64 is an independent fp64
projection (SetWindow, SphericalTo2D from the fp32 window and the fp32 grid angles, every later
operation in fp64) that pins it away from the window edges and the pixel boundaries, and serves the
CPU tests as a table of its own.
"""
import math

import numpy as np

import planar_ref as P
import pf_layouts as PL

f32 = np.float32
NAN = float("nan")
_IDX = ((0, 1, 2, 3), (1, 4, 5, 6), (2, 5, 7, 8), (3, 6, 8, 9))


def clamp(v):
    """clamp_sample: (double)v into [1e-4, 1 - 1e-4]; NaN stays."""
    v = np.asarray(v, np.float64).copy()
    lo = v < 1e-4
    hi = ~lo & (v > (1 - 1e-4))
    v[lo] = 1e-4
    v[hi] = 1 - 1e-4
    return v


# ---- the moment sums ----------------------------------------------------------------------------
def _upper10(X):
    X2 = X * X
    X3 = X * X * X
    return X2, X3, [X3 * X3, X3 * X2, X3 * X, X3, X2 * X2, X2 * X, X2, X * X, X, np.ones_like(X)]


def data_sums(xs, ys):
    """k_register's 15 sums of already clamped fp64 samples."""
    X = np.asarray(xs, np.float64)
    y = np.asarray(ys, np.float64)
    X2, X3, up = _upper10(X)
    return P.ordered_sums(np.stack(up + [X3 * y, X2 * y, X * y, y, y * y], 1))


def pair_sums(vp, vq):
    """k_pair_moments' 36 sums from the raw float32 values of the pair's samples in tile p / q."""
    if len(vp) == 0:
        return np.zeros(36)
    X, Z = clamp(vp), clamp(vq)
    X2, X3, U = _upper10(X)
    Z2, Z3, V = _upper10(Z)
    one = np.ones_like(X)
    C = [X3 * Z3, X3 * Z2, X3 * Z, X3, X2 * Z3, X2 * Z2, X2 * Z, X2, X * Z3, X * Z2, X * Z, X,
         Z3, Z2, Z, one]
    with np.errstate(invalid="ignore"):
        return P.ordered_sums(np.stack(U + V + C, 1))


def pair_values(tile_off, data, pairs, index):
    """Per pair the raw float32 values (in tile p, in tile q) of its samples.  tile_off: element
    offset of every tile inside data; pairs [np][4] = {p, q, first, count}; index [ns][2]."""
    out = []
    for p, q, first, count in np.asarray(pairs).tolist():
        ix = np.asarray(index)[first:first + count]
        out.append((data[tile_off[p] + ix[:, 0]], data[tile_off[q] + ix[:, 1]]))
    return out


# ---- assemble and solve -------------------------------------------------------------------------
def assemble(D, Pm, pairs, lam):
    """(A [n][n] with its lower triangle set, r [n]) from the data sums D [nt][15], the pair sums
    Pm [np][36] and the pair list."""
    nt = len(D)
    n = 4 * nt
    A = np.zeros((n, n), np.float64)
    r = np.zeros(n, np.float64)
    pairs = [tuple(int(v) for v in row[:2]) for row in np.asarray(pairs).reshape(-1, 4)]
    where = {pq: i for i, pq in enumerate(pairs)}
    lam = float(lam)
    for p in range(nt):
        blk = np.array(D[p][:10], np.float64)
        for i, (a, _) in enumerate(pairs):
            if a == p:
                blk = blk + lam * Pm[i][0:10]
        for i, (_, b) in enumerate(pairs):
            if b == p:
                blk = blk + lam * Pm[i][10:20]
        for i in range(4):
            for j in range(i + 1):
                A[4 * p + i, 4 * p + j] = blk[_IDX[i][j]]
            r[4 * p + i] = D[p][10 + i]
    zero = np.zeros((4, 4))
    for (p, q) in pairs:
        if p < q and (q, p) in where:
            continue
        a, b = max(p, q), min(p, q)
        cab = Pm[where[(a, b)]][20:36].reshape(4, 4) if (a, b) in where else zero
        cba = Pm[where[(b, a)]][20:36].reshape(4, 4) if (b, a) in where else zero
        with np.errstate(invalid="ignore"):
            A[4 * a:4 * a + 4, 4 * b:4 * b + 4] = -(lam * (cab + cba.T))
    return A, r


def cholesky_solve(A, r):
    """The solution of A c = r by the kernel's factorisation and substitutions, or None."""
    A = np.array(A, np.float64)
    n = A.shape[0]
    with np.errstate(all="ignore"):
        for k in range(n):
            if not A[k, k] > 0.0:
                return None
            d = math.sqrt(A[k, k])
            A[k, k] = d
            A[k + 1:, k] = A[k + 1:, k] / d
            col = A[k + 1:, k].copy()
            A[k + 1:, k + 1:] = A[k + 1:, k + 1:] - np.outer(col, col)
        b = np.array(r, np.float64)
        z = np.zeros(n)
        for k in range(n):
            z[k] = b[k] / A[k, k]
            b[k + 1:] = b[k + 1:] - A[k + 1:, k] * z[k]
        c = np.zeros(n)
        for k in range(n - 1, -1, -1):
            c[k] = z[k] / A[k, k]
            z[:k] = z[:k] - A[k, :k] * c[k]
    return c if np.isfinite(c).all() else None


def _quad4(S, c, d):
    acc = 0.0
    for i in range(4):
        t = 0.0
        for j in range(4):
            t = t + float(S[i][j]) * float(d[j])
        acc = acc + float(c[i]) * t
    return acc


def _sym(s10):
    return [[s10[_IDX[i][j]] for j in range(4)] for i in range(4)]


def costs(D, Pm, pairs, c):
    """(data cost, pair cost without the factor lam) at c [nt][4], from the moment sums."""
    dc = 0.0
    for p in range(len(D)):
        S = D[p]
        cJy = 0.0
        for i in range(4):
            cJy = cJy + float(c[p][i]) * float(S[10 + i])
        dc = dc + ((float(S[14]) - 2.0 * cJy) + _quad4(_sym(S[0:10]), c[p], c[p]))
    pc = 0.0
    for i, row in enumerate(np.asarray(pairs).reshape(-1, 4).tolist()):
        p, q = row[0], row[1]
        S = Pm[i]
        cUc = _quad4(_sym(S[0:10]), c[p], c[p])
        dVd = _quad4(_sym(S[10:20]), c[q], c[q])
        cCd = _quad4(S[20:36].reshape(4, 4), c[p], c[q])
        pc = pc + ((cUc - 2.0 * cCd) + dVd)
    return dc, pc


def register(D, Pm, pairs, lam):
    """pf_register_consistent of one panorama: (coeffs64 [nt][4], summary [4])."""
    nt = len(D)
    nsamp = float(sum(int(row[3]) for row in np.asarray(pairs).reshape(-1, 4)))
    A, r = assemble(D, Pm, pairs, lam)
    c = cholesky_solve(A, r)
    if c is None:
        return np.full((nt, 4), NAN), np.array([NAN, NAN, nsamp, 1.0])
    c = c.reshape(nt, 4)
    dc, pc = costs(D, Pm, pairs, c)
    return c, np.array([dc, pc, nsamp, 0.0])


# ---- the fp32 transform and the overlap statistics ----------------------------------------------
def cubic_map(v, abcd):
    """Depth2DepthTransform's per-pixel map in fp32 (cubic_map of csrc/pf_internal.hpp)."""
    X = P._clamp_x(v)
    a, b, c, d = [f32(t) for t in np.asarray(abcd, f32)]
    with np.errstate(all="ignore"):
        Y = (a * X * X * X + b * X * X + c * X + d).astype(f32)
        neg = Y < 0
        big = ~neg & (Y > 1)
    Y[neg] = f32(0)
    Y[big] = f32(1)
    return Y


def overlap_stats(values, pairs, coeffs=None):
    """[np][5] from pair_values' output; coeffs: None or float32 [nt][4]."""
    out = np.zeros((len(values), 5), np.float64)
    for i, (vp, vq) in enumerate(values):
        p, q = int(pairs[i][0]), int(pairs[i][1])
        if coeffs is not None:
            vp, vq = cubic_map(vp, coeffs[p]), cubic_map(vq, coeffs[q])
        ok = ~(np.isnan(vp) | np.isnan(vq))
        d = np.where(ok, vp.astype(np.float64) - vq.astype(np.float64), 0.0)
        T = np.stack([ok.astype(np.float64), d, d * d, (~ok).astype(np.float64)], 1)
        s = P.ordered_sums(T) if len(d) else np.zeros(4)
        out[i] = [s[0], s[1], s[2], np.abs(d).max() if len(d) else 0.0, s[3]]
    return out


def overlap_rms(stats):
    """sqrt(sum sum d^2 / sum count) over all pairs of [..., np, 5] statistics."""
    stats = np.asarray(stats)
    return math.sqrt(stats[..., 2].sum() / stats[..., 0].sum())


# ---- the independent fp64 projection ------------------------------------------------------------
def _unit(v):
    return v / math.sqrt(float(v @ v))


def window64(fov):
    """SetWindow (Depth.cpp:120-155) in fp64 from the fp32 window: (middle, hedge, vedge, corner0)."""
    aL, aR, zT, zD = [float(f32(v)) for v in fov]
    az, zen = (aL + aR) / 2, (zT + zD) / 2
    mid = np.array([math.sin(zen) * math.cos(az), math.sin(zen) * math.sin(az), math.cos(zen)])
    left = _unit(np.cross([0.0, 0.0, 1.0], mid))
    up = _unit(np.cross(left, mid))
    ta, tz = math.tan(abs(aR - aL) / 2), math.tan(abs(zT - zD) / 2)
    lm, rm = mid + left * ta, mid - left * ta
    um, dm = mid - up * tz, mid + up * tz
    return mid, rm - lm, dm - um, mid + (lm - mid) + (um - mid)


def project64(win, az, zen):
    """SphericalTo2D (Depth.cpp:168-182) in fp64 on arrays of angles: (x, y, den)."""
    mid, he, ve, c0 = win
    d = np.stack([np.sin(zen) * np.cos(az), np.sin(zen) * np.sin(az), np.cos(zen)], -1)
    den = d @ mid
    with np.errstate(all="ignore"):
        pos = d * ((mid @ mid) / den)[..., None]
    e = pos - c0
    return (e @ he) / (he @ he), (e @ ve) / (ve @ ve), den


def reg_grid(rng, zr):
    """The registration grid of a tile (Depth.cpp:1298-1335) as fp32 angles: (az [ns], zen [ns]),
    rows of cols + 1 samples, as k_register walks them."""
    r0, r1, r2, r3 = [f32(v) for v in rng]
    subd = f32(1 / 180.0 * PL.MYPI)
    cols = int(math.floor(float(np.abs(f32(r1 - r0)) / subd) + 0.5))  # roundf: halves away from 0
    top = max(f32(zr[0]), r2)
    down = min(f32(zr[1]), r3)
    rows = int(math.floor(float(np.abs(f32(down - top)) / subd) + 0.5))
    az = (r0 + f32(r1 - r0) * np.arange(cols + 1, dtype=f32) / f32(cols)).astype(f32)
    zen = (top + f32(down - top) * np.arange(rows + 1, dtype=f32) / f32(rows)).astype(f32)
    return np.tile(az, rows + 1), np.repeat(zen, cols + 1)


def reg_grid64(rng, zr):
    """The same grid with every operation after the fp32 ranges in fp64.  Where a range is a
    whole number of degrees plus a half (C2's 32.5-degree bands) fp32 and fp64 round the row count
    differently, so this grid can differ from the kernels' by a row."""
    r0, r1, r2, r3 = [float(f32(v)) for v in rng]
    subd = 1 / 180.0 * PL.MYPI
    cols = int(math.floor(abs(r1 - r0) / subd + 0.5))
    top = max(float(f32(zr[0])), r2)
    down = min(float(f32(zr[1])), r3)
    rows = int(math.floor(abs(down - top) / subd + 0.5))
    az = r0 + (r1 - r0) * np.arange(cols + 1) / cols
    zen = top + (down - top) * np.arange(rows + 1) / rows
    return np.tile(az, rows + 1), np.repeat(zen, cols + 1)


def elem64(x, y, w, h, c):
    """Value()'s element at fp64 (x, y) already inside [0, 1]."""
    X = (x * (w - 1)).astype(np.int64)
    Y = (y * (h - 1)).astype(np.int64)
    return (Y * w + X) * c


def projections64(layout, zr, grid=reg_grid):
    """{(p, q): (x, y, den)} of every sample of tile p projected into tile q (q == p included),
    with the capped ranges MergeDepthMaps registers with.  grid: reg_grid (the kernels' samples)
    or reg_grid64."""
    rng = layout.capped_ranges()
    wins = [window64(layout.fovs[p]) for p in range(layout.ntiles)]
    out = {}
    for p in range(layout.ntiles):
        az, zen = grid(rng[p], zr)
        az, zen = az.astype(np.float64), zen.astype(np.float64)
        for q in range(layout.ntiles):
            out[(p, q)] = project64(wins[q], az, zen)
    return out


def inside64(x, y, den, lo=0.0, hi=1.0):
    with np.errstate(invalid="ignore"):
        return (den > 0) & (x >= lo) & (x <= hi) & (y >= lo) & (y <= hi)


def pair_table64(layout, zr, channels=1, grid=reg_grid):
    """The pair table by the fp64 projection alone: (pairs [np][4], index [ns][2])."""
    proj = projections64(layout, zr, grid)
    pairs, index, first = [], [], 0
    for p in range(layout.ntiles):
        xp, yp, _ = proj[(p, p)]
        ep = elem64(np.clip(xp, 0.0, 1.0), np.clip(yp, 0.0, 1.0), int(layout.tile_w[p]),
                    int(layout.tile_h[p]), channels)
        for q in range(layout.ntiles):
            if q == p:
                continue
            x, y, den = proj[(p, q)]
            keep = inside64(x, y, den)
            n = int(keep.sum())
            if n == 0:
                continue
            eq = elem64(x[keep], y[keep], int(layout.tile_w[q]), int(layout.tile_h[q]), channels)
            pairs.append((p, q, first, n))
            index.append(np.stack([ep[keep], eq], 1))
            first += n
    return np.array(pairs, np.int64).reshape(-1, 4), (np.concatenate(index) if index
                                                      else np.zeros((0, 2), np.int64))


def tile_offsets(layout, channels=1):
    off, out = 0, []
    for w, h in zip(layout.tile_w, layout.tile_h):
        out.append(off)
        off += int(w) * int(h) * channels
    return out
