"""The sharded fusion's level and band calls (csrc/pf_shard.hip) and its two flows
(pf_dist.fuse_row_sharded, fuse_tile_sharded) at the rows of tests/shard_shapes.py, bit for bit
against the CPU oracle and the one-GPU pf_fuse.

tests/test_gpu_rowshard.py runs the flows at C2 and C5 only: widths 512 .. 8192, height = width / 2,
the band layouts, every level with the coverage certificate.  The table (checked on the CPU in
tests/test_shard_shapes.py) adds what those never reach: a partial patch column together with a
row cut in the middle of a patch in the partial-sum kernel, band passes on 124 and 126 columns,
on the general form, after a baseline that does not divide the level and after the upsample of an
odd-width level, the scalar form of the border kernel, the per-sweep engine in pf_fuse_level and
pf_fuse_finish_level, the multicover fix-up on a layout with pixels covered four times, ranks
without a tile, and heights other than width / 2.

a. The pieces on one context, for every case and level; output planes start as a NaN sentinel, so
   a row written outside the asked range, or left unwritten inside it, shows.
b. The flows on thread-simulated ranks (tests/shard_sim.py) for every (case, world, rep_levels):
   rank 0's u16 equals pf_fuse's and the oracle's.
c. Where a level's bands would be thinner than the halo the flow refuses: a ValueError on every
   rank before any exchange.  Which (case, world) pairs refuse follows from the device's pass
   plans through pf_dist.level_geometry; worlds 1 and 2 never do, and only worlds >= 5 may.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import panofuse  # noqa: E402
import pf_dist  # noqa: E402
import pyoracle as O  # noqa: E402
import shard_shapes as S  # noqa: E402
from shard_sim import run_ranks  # noqa: E402

DEV = "cuda:0"
SENT = 0x7FC0BEEF  # a quiet NaN no kernel writes: not the targets' un-windowed marker, not a sum
CASE_NAMES = [c["name"] for c in S.CASES]
_DEVICE = {}
_ORACLE = {}


@pytest.fixture(scope="module")
def fuser():
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected on a host without a GPU")
    f = panofuse.Fuser(0)
    yield f
    f.close()


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # a copy: the shared inputs are read-only


def _sent(n):
    return torch.full((n,), SENT, dtype=torch.int32, device=DEV).view(torch.float32)


def _bits(t, L=None):
    a = t.detach().cpu().numpy().view(np.int32)
    return a if L is None else a.reshape(L.h, L.w)


def _fbits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _case(name):
    """The case's inputs on the device, uploaded once."""
    if name not in _DEVICE:
        k = S.inputs(name)
        _DEVICE[name] = dict(k, tiles_d=_dev(k["data"])[None].contiguous(),
                             coeffs_d=_dev(k["coeffs"]), emap_d=_dev(k["emap"])[None].contiguous())
    return _DEVICE[name]


def _args(k):
    c = k["case"]
    return c["out_w"], c["out_h"], c["zr"]


def _subset(name, lv, t0, t1, xform):
    """The oracle's (sum, count) of tiles [t0, t1) at a level: of the transformed tile data, or
    of the data as it is.  Computed once."""
    key = (name, lv, t0, t1, xform)
    if key not in _ORACLE:
        k = S.inputs(name)
        L = S.level(k["case"], lv)
        if t1 > t0:
            ls, n = O.targets_subset(k["tiles"], t0, t1, k["xdata"] if xform else k["data"], L)
        else:
            ls, n = np.zeros((L.h, L.w), np.float32), np.zeros((L.h, L.w), np.int32)
        _ORACLE[key] = (_fbits(ls), _fbits(n.astype(np.float32)))
    return _ORACLE[key]


def _row_ranges(L):
    """The band; a range that cuts two patches of the partial-sum kernel; one row; the whole
    level, rows outside the band included."""
    return [(L.h0, L.h1 + 1), (L.h0 + 3, L.h0 + 13), (L.h0 + 5, L.h0 + 6), (0, L.h)]


def _tile_ranges(nt):
    return [(0, nt), (0, nt // 2), (nt // 2, nt // 2)]


def _outside_intact(got, a, b):
    return bool((got[:a] == SENT).all() and (got[b:] == SENT).all())


def _gpu_fuse(fuser, k):
    """pf_fuse's u16 panorama of the case (the layout set on `fuser`), once."""
    if "fused" not in k:
        w, h, zr = _args(k)
        out = torch.zeros((1, h, w), dtype=torch.int16, device=DEV)
        fuser.fuse(k["emap_d"], k["tiles_d"], out, zr, coeffs=k["coeffs_d"][None].contiguous())
        fuser.synchronize()
        k["fused"] = out.cpu().numpy().view(np.uint16)[0]
    return k["fused"]


# ---- a. the pieces ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_one_gpu_fuse_equals_oracle(fuser, name):
    """The yardstick of the flows: pf_fuse at the case equals the oracle."""
    k = _case(name)
    fuser.set_tiles(k["lay"])
    got, ref = _gpu_fuse(fuser, k), S.reference(name)
    bad = int((got != ref).sum())
    assert bad == 0, f"{name}: {bad} pixels differ from the oracle"
    assert np.count_nonzero(ref) > k["case"]["out_w"]


def test_refused_size(fuser):
    """500x250 (level 0 125x62, level 1 250x125) is no size pf_fuse takes: the table has 500x248."""
    k = _case("c1-500x248")
    fuser.set_tiles(k["lay"])
    w, h = S.REFUSED_SIZE
    out = torch.zeros((1, h, w), dtype=torch.int16, device=DEV)
    with pytest.raises(panofuse.PanofuseError, match="not divisible"):
        fuser.fuse(k["emap_d"], k["tiles_d"], out, S.ZR)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_partial_sums(fuser, name):
    """pf_fuse_partial_rows and pf_fuse_partial: sums and counts of all tiles, half of them and
    none, with the fused transform and without, on four row ranges and on the whole plane."""
    k = _case(name)
    fuser.set_tiles(k["lay"])
    w, h, zr = _args(k)
    nt = k["lay"].ntiles
    for lv in range(S.nlevels(k["case"])):
        L = S.level(k["case"], lv)
        for t0, t1 in _tile_ranges(nt):
            for xform in (True, False):
                cf = k["coeffs_d"] if xform else None
                ref_l, ref_n = _subset(name, lv, t0, t1, xform)
                tag = f"{name} level {lv} tiles [{t0},{t1}) xform {xform}"
                for a, b in _row_ranges(L):
                    lsum, cnt = _sent(L.w * L.h), _sent(L.w * L.h)
                    fuser.fuse_partial_rows(k["tiles_d"], cf, t0, t1, w, zr, lv, a, b, lsum, cnt,
                                            out_h=h)
                    fuser.synchronize()
                    gl, gn = _bits(lsum, L), _bits(cnt, L)
                    assert np.array_equal(gn[a:b], ref_n[a:b]), f"{tag} rows [{a},{b}): counts"
                    bad = np.nonzero((gl[a:b] != ref_l[a:b]).any(1))[0]
                    assert bad.size == 0, f"{tag} rows [{a},{b}): sums differ in rows {a + bad}"
                    assert _outside_intact(gl, a, b) and _outside_intact(gn, a, b), \
                        f"{tag}: rows outside [{a},{b}) written"
                    # rows of the range outside the band: zero sums and counts
                    out_band = np.r_[a:min(b, L.h0), max(a, L.h1 + 1):b]
                    assert not gl[out_band].any() and not gn[out_band].any(), tag
                lsum, cnt = _sent(L.w * L.h), _sent(L.w * L.h)
                fuser.fuse_partial(k["tiles_d"], cf, t0, t1, w, zr, lv, lsum, cnt, out_h=h)
                fuser.synchronize()
                assert np.array_equal(_bits(cnt, L), ref_n), f"{tag}: pf_fuse_partial counts"
                assert np.array_equal(_bits(lsum, L), ref_l), f"{tag}: pf_fuse_partial sums"
        assert int(_subset(name, lv, 0, nt, True)[1].max()) > 0


@pytest.mark.parametrize("name", CASE_NAMES)
def test_coverage_normalize_and_tile_rows(fuser, name):
    k = _case(name)
    fuser.set_tiles(k["lay"])
    w, h, zr = _args(k)
    nt = k["lay"].ntiles
    for lv in range(S.nlevels(k["case"])):
        L = S.level(k["case"], lv)
        ref_l, ref_n = _subset(name, lv, 0, nt, True)
        n_int = ref_n.view(np.float32).astype(np.int32)
        ref_norm = _fbits(O.normalize(ref_l.view(np.float32), n_int, L))
        lsum, cnt = _sent(L.w * L.h), _sent(L.w * L.h)
        fuser.fuse_partial(k["tiles_d"], k["coeffs_d"], 0, nt, w, zr, lv, lsum, cnt, out_h=h)
        tgt = _sent(L.w * L.h)
        fuser.fuse_targets(k["tiles_d"], k["coeffs_d"], w, zr, lv, tgt, out_h=h)
        fuser.synchronize()
        g_tgt = _bits(tgt, L)
        band = slice(L.h0, L.h1 + 1)
        assert np.array_equal(g_tgt[band], ref_norm[band]), f"{name} level {lv}: pf_fuse_targets"
        for a, b in _row_ranges(L):
            tag = f"{name} level {lv} rows [{a},{b})"
            cov = _sent(L.w * L.h)
            fuser.fuse_coverage_rows(w, zr, lv, a, b, cov, out_h=h)
            lnorm = _sent(L.w * L.h)
            fuser.fuse_normalize_rows(lsum, cnt, w, zr, lv, a, b, lnorm, out_h=h)
            fuser.synchronize()
            g_cov, g_norm = _bits(cov, L), _bits(lnorm, L)
            assert np.array_equal(g_cov[a:b], ref_n[a:b]), f"{tag}: coverage"
            assert _outside_intact(g_cov, a, b), f"{tag}: coverage rows outside written"
            assert np.array_equal(g_norm[a:b], ref_norm[a:b]), f"{tag}: normalize_rows vs oracle"
            ia, ib = max(a, L.h0), min(b, L.h1 + 1)
            assert np.array_equal(g_norm[ia:ib], g_tgt[ia:ib]), f"{tag}: normalize_rows vs targets"
            assert _outside_intact(g_norm, a, b), f"{tag}: normalize rows outside written"
        lnorm = _sent(L.w * L.h)
        fuser.fuse_normalize(lsum, cnt, w, zr, lv, lnorm, out_h=h)
        fuser.synchronize()
        g_norm = _bits(lnorm, L)
        assert np.array_equal(g_norm[band], ref_norm[band]), f"{name} level {lv}: pf_fuse_normalize"
        assert _outside_intact(g_norm, L.h0, L.h1 + 1)
        # the rows a rank's tiles may feed: inside h0+1 .. h1-1, and every row the oracle counts
        ranges = set(_tile_ranges(nt))
        for world in k["case"]["worlds"]:
            ranges |= {pf_dist.shard_range(nt, r, world) for r in range(world)}
        for t0, t1 in sorted(ranges):
            ymin, ymax = fuser.fuse_tile_rows(w, zr, lv, t0, t1, out_h=h)
            rows = np.nonzero(_subset(name, lv, t0, t1, True)[1].any(1))[0]
            tag = f"{name} level {lv} tiles [{t0},{t1}): rows {ymin}..{ymax}"
            if t0 == t1:
                assert ymin > ymax, tag
            if ymin <= ymax:
                assert L.h0 + 1 <= ymin and ymax <= L.h1 - 1, tag
            if rows.size:
                assert ymin <= rows[0] and rows[-1] <= ymax, f"{tag}, the oracle's {rows[0]}..{rows[-1]}"


def test_multicover_fixup_edge_layout(fuser):
    """Pixels covered by three and four tiles: the count of (pixel, tile) pairs, and the summed
    per-range terms patched into the summed per-range planes give the all-tile sums."""
    name = "edge-512x256"
    k = _case(name)
    fuser.set_tiles(k["lay"])
    w, h, zr = _args(k)
    nt = k["lay"].ntiles
    for lv in range(S.nlevels(k["case"])):
        L = S.level(k["case"], lv)
        ref_l, ref_n = _subset(name, lv, 0, nt, True)
        n = ref_n.view(np.float32)
        npairs = fuser.multicover_count(w, zr, lv, out_h=h)
        assert npairs == int(n[n >= 3].sum()) > 0, f"level {lv}"
        total = torch.zeros(L.w * L.h, dtype=torch.float32, device=DEV)
        terms = torch.zeros(npairs, dtype=torch.float32, device=DEV)
        for r in range(3):
            t0, t1 = pf_dist.shard_range(nt, r, 3)
            lsum, cnt = _sent(L.w * L.h), _sent(L.w * L.h)
            fuser.fuse_partial(k["tiles_d"], k["coeffs_d"], t0, t1, w, zr, lv, lsum, cnt, out_h=h)
            part = _sent(npairs)
            fuser.multicover(k["tiles_d"], k["coeffs_d"], t0, t1, w, zr, lv, part, out_h=h)
            fuser.synchronize()
            total += lsum
            terms += part
        torch.cuda.synchronize()
        fuser.multicover_patch(w, zr, lv, terms, total, out_h=h)
        fuser.synchronize()
        got = _bits(total, L)
        bad = int((got != ref_l).sum())
        assert bad == 0, f"level {lv}: {bad} sums differ from the all-tile sums after the patch"
        assert int((got != ref_l)[n < 3].sum()) == 0
    for other in ("c1-600x300", "holes-600x300"):
        ko = _case(other)
        fuser.set_tiles(ko["lay"])
        wo, ho, zo = _args(ko)
        assert [fuser.multicover_count(wo, zo, lv, out_h=ho) for lv in range(3)] == [0, 0, 0]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_level_forms_and_band_passes(fuser, name):
    """Per level: pf_fuse_seed + pf_fuse_finish_level, pf_fuse_level on (lsum, cnt) and
    pf_fuse_level on pf_fuse_targets' plane agree plane by plane (levels on the per-sweep engine
    included); where the level has band passes, pf_fuse_border + the passes of pf_fuse_band_plan
    over the whole band give the same plane, or the same u16 on the last level.  The u16 of every
    form equals pf_fuse's and the oracle's."""
    k = _case(name)
    case = k["case"]
    fuser.set_tiles(k["lay"])
    w, h, zr = _args(k)
    nt = k["lay"].ntiles
    nlev = S.nlevels(case)
    forms = ("seed+finish", "level", "level-targets", "passes")
    prev = {f: None for f in forms}
    outs = {f: torch.zeros(w * h, dtype=torch.int16, device=DEV) for f in forms}
    swept = []
    for lv in range(nlev):
        L = S.level(case, lv)
        last = lv == nlev - 1
        n = L.w * L.h
        lsum, cnt, tgt = _sent(n), _sent(n), _sent(n)
        fuser.fuse_partial(k["tiles_d"], k["coeffs_d"], 0, nt, w, zr, lv, lsum, cnt, out_h=h)
        fuser.fuse_targets(k["tiles_d"], k["coeffs_d"], w, zr, lv, tgt, out_h=h)
        bufs = {f: _sent(n) for f in forms}
        e = k["emap_d"] if lv == 0 else None
        o = {f: outs[f].view(L.h, L.w) if last else None for f in forms}
        fuser.fuse_seed(e, prev["seed+finish"], w, zr, lv, bufs["seed+finish"], out_h=h)
        fuser.fuse_finish_level(lsum, cnt, w, zr, lv, bufs["seed+finish"], o["seed+finish"],
                                out_h=h)
        fuser.fuse_level(e, prev["level"], lsum, cnt, w, zr, lv, bufs["level"], o["level"],
                         out_h=h)
        fuser.fuse_level(e, prev["level-targets"], tgt, None, w, zr, lv, bufs["level-targets"],
                         o["level-targets"], out_h=h)
        fuser.synchronize()
        npass = fuser.band_pass_count(w, zr, lv, 1, out_h=h)
        assert (npass == 0) == (lv in case["sweeps"]), f"{name} level {lv}: {npass} band passes"
        if npass:
            plan = fuser.fuse_band_plan(w, zr, lv, 1, out_h=h)
            assert len(plan) == npass and sum(plan) == L.iters, plan
            a, b = _sent(n), _sent(n)
            pv = prev["passes"]
            if last:
                fuser.fuse_border(pv, w, zr, lv, a=a, b=b, out=outs["passes"], out_h=h)
            else:
                fuser.fuse_border(pv, w, zr, lv, a=a, b=b, out_h=h)
            src, dst = None, a
            for i, T in enumerate(plan):
                mode = (2 if lv == 0 else 1) if i == 0 else 0
                fin = last and i == len(plan) - 1
                fuser.fuse_band_pass(tgt, mode, w, zr, lv, T, L.h0, L.h1 + 1,
                                     src=src if mode == 0 else None, dst=None if fin else dst,
                                     prev=pv if mode == 1 else None, emap=e if mode == 2 else None,
                                     out=outs["passes"] if fin else None, out_h=h)
                src, dst = dst, (b if dst is a else a)
            fuser.synchronize()
            bufs["passes"] = src
            swept.append(lv)
        else:
            with pytest.raises(panofuse.PanofuseError, match="no band passes at width"):
                fuser.fuse_band_plan(w, zr, lv, 1, out_h=h)
            bufs["passes"] = bufs["level"]  # the next level's passes start from this one
        if not last:
            ref = _bits(bufs["seed+finish"], L)
            assert not (ref == SENT).any(), f"{name} level {lv}: unwritten values"
            for f in forms[1:]:
                bad = np.nonzero((_bits(bufs[f], L) != ref).any(1))[0]
                assert bad.size == 0, (f"{name} level {lv}: {f} differs from seed+finish in rows "
                                       f"{bad[:20]} (band {L.h0}..{L.h1})")
        prev = bufs
    assert swept and nlev - 1 in swept
    ref = S.reference(name)
    fused = _gpu_fuse(fuser, k)
    for f in forms:
        got = outs[f].cpu().numpy().view(np.uint16).reshape(h, w)
        bad = np.nonzero((got != fused).any(1))[0]
        assert bad.size == 0, f"{name}: {f} differs from pf_fuse in rows {bad[:20]}"
        assert np.array_equal(got, ref), f"{name}: {f} differs from the oracle"
    assert fuser.jres_errors() == 0


# ---- b, c. the flows ----------------------------------------------------------------------------
def _predict(fuser, k, world, rep):
    """(rep_levels in effect, the first level whose bands are thinner than its halo or None): the
    flow's own rules -- a level without band passes is replicated, a row-sharded level takes
    pf_dist.level_geometry of the device's plan -- on a backend of the main context."""
    w, h, zr = _args(k)
    nt = k["lay"].ntiles
    be = pf_dist.HipRowShardBackend(fuser, k["emap_d"], k["tiles_d"], k["coeffs_d"], w, zr, None,
                                    out_h=h)
    if rep == "auto":
        rep = pf_dist.auto_rep_levels(be, be.nlevels, world)
    if world == 1:
        return be.nlevels, None
    nrep = rep
    for lv in range(be.nlevels):
        if lv < nrep:
            continue
        plan = be.plan(lv, world)
        if not plan:
            assert lv == nrep, "levels without band passes are the coarsest ones"
            nrep = lv + 1
            continue
        _, _, h0, h1 = be.dims(lv)
        ext = [be.tile_rows(lv, *pf_dist.shard_range(nt, r, world)) for r in range(world)]
        _, K, bnd = pf_dist.level_geometry(h0, h1, world, ext, plan)
        if min(bnd[r + 1] - bnd[r] for r in range(world)) < K:
            return nrep, lv
    return nrep, None


def _run_rows(k, world, rep, side=False):
    """fuse_row_sharded on `world` threads, a context per rank: (rank 0's u16, errors, logs)."""
    w, h, zr = _args(k)
    lay = k["lay"]
    logs = [pf_dist.ExchangeLog() for _ in range(world)]

    def body(r, comm):
        f = panofuse.Fuser(0)
        fs = None
        try:
            f.set_tiles(lay)
            out = torch.zeros(w * h, dtype=torch.int16, device=DEV)
            be = pf_dist.HipRowShardBackend(f, k["emap_d"], k["tiles_d"], k["coeffs_d"], w, zr,
                                            out, out_h=h)
            if side:
                fs = panofuse.Fuser(0, stream=torch.cuda.Stream(DEV))
                fs.set_tiles(lay)
                be.enable_side(fs)
            n = rep
            if rep == "auto":  # rank 0's answer on every rank
                n = pf_dist.auto_rep_levels(be, be.nlevels, world, comm=comm)
            pf_dist.fuse_row_sharded(be, be.nlevels, lay.ntiles, r, world, comm, logs[r],
                                     rep_levels=n)
            torch.cuda.synchronize()
            return out.cpu().numpy().view(np.uint16).reshape(h, w)
        finally:
            torch.cuda.synchronize()
            if fs is not None:
                fs.close()
            f.close()

    outs, errs = run_ranks(world, body)
    return outs[0], errs, logs


def _check_rows(fuser, name, world, rep, side=False):
    k = _case(name)
    fuser.set_tiles(k["lay"])
    nrep, thin = _predict(fuser, k, world, rep)
    fused = _gpu_fuse(fuser, k)
    got, errs, logs = _run_rows(k, world, rep, side)
    tag = f"{name} world {world} rep {rep} (in effect {nrep})"
    if thin is not None:
        # c. the refusal: on every rank, before any exchange; never at worlds 1 and 2, and only
        # from 5 ranks on in this table
        assert world >= 5, f"{tag}: level {thin} refused"
        assert all(isinstance(e, ValueError) and "thinner than" in str(e) for e in errs), errs
        assert all(not log.sent and log.rounds == 0 for log in logs), [log.sent for log in logs]
        print(f"thin-band refusal: {tag} at level {thin}")
        return
    assert not any(errs), (tag, errs)
    bad = np.nonzero((got != fused).any(1))[0]
    assert bad.size == 0, f"{tag}: rank 0 differs from pf_fuse in rows {bad[:20]}"
    assert np.array_equal(got, S.reference(name)), f"{tag}: rank 0 differs from the oracle"
    if world > 1 and nrep < 3:
        assert all(log.sent.get("targets", 0) > 0 or log.rounds > 0 for log in logs)


ROW_FLOWS = [(c["name"], world, rep) for c in S.CASES for world in c["worlds"]
             for rep in (c["reps"] if world > 1 else c["reps"][:1])]


@pytest.mark.parametrize("name,world,rep", ROW_FLOWS,
                         ids=[f"{n}-w{w}-rep{r}" for n, w, r in ROW_FLOWS])
def test_row_sharded_flow(fuser, name, world, rep):
    _check_rows(fuser, name, world, rep)


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", S.SIDE_CASES)
def test_row_sharded_flow_side_stream(fuser, name, world):
    """Level 0 replicated and the finer levels' tile sums on a second stream beside its sweeps."""
    _check_rows(fuser, name, world, 1, side=True)


TILE_FLOWS = [(c["name"], world) for c in S.CASES for world in c["worlds"]]


@pytest.mark.parametrize("name,world", TILE_FLOWS, ids=[f"{n}-w{w}" for n, w in TILE_FLOWS])
def test_tile_sharded_flow(fuser, name, world):
    """fuse_tile_sharded (rank 0 sweeps; the multicover fix-up on the edge layout; ranks without
    a tile at worlds 7 and 9): rank 0's u16 equals pf_fuse's and the oracle's."""
    k = _case(name)
    fuser.set_tiles(k["lay"])
    fused = _gpu_fuse(fuser, k)
    w, h, zr = _args(k)
    lay = k["lay"]

    def body(r, comm):
        f = panofuse.Fuser(0)
        try:
            f.set_tiles(lay)
            out = torch.zeros((h, w), dtype=torch.int16, device=DEV)
            be = pf_dist.HipTileShardBackend(f, k["emap_d"], k["tiles_d"], k["coeffs_d"], w, zr,
                                             out, out_h=h)
            pf_dist.fuse_tile_sharded(be, S.nlevels(k["case"]), lay.ntiles, r, world, comm)
            torch.cuda.synchronize()
            return out.cpu().numpy().view(np.uint16)
        finally:
            torch.cuda.synchronize()
            f.close()

    outs, errs = run_ranks(world, body)
    assert not any(errs), errs
    bad = np.nonzero((outs[0] != fused).any(1))[0]
    assert bad.size == 0, f"{name} world {world}: rank 0 differs from pf_fuse in rows {bad[:20]}"
    assert np.array_equal(outs[0], S.reference(name))


def test_refusals_only_from_five_ranks_on(fuser):
    """Over the whole table: every case runs the full flow at worlds 1 and 2 with rep_levels 0
    (or with the levels without band passes replicated), and at most worlds >= 5 refuse."""
    refused = []
    for c in S.CASES:
        k = _case(c["name"])
        fuser.set_tiles(k["lay"])
        for world in c["worlds"]:
            for rep in c["reps"]:
                nrep, thin = _predict(fuser, k, world, rep)
                if world <= 2 and rep == 0:
                    assert thin is None and nrep == (3 if world == 1 else len(c["sweeps"]))
                if thin is not None:
                    refused.append((c["name"], world, rep, thin))
    assert all(world >= 5 for _, world, _, _ in refused), refused
    print("thin-band refusals (case, world, rep_levels, level):", refused)
