"""tests/shard_shapes.py's table, checked on the CPU: every row is what it is listed for, and
the orchestration of pf_dist.fuse_row_sharded -- a level without band passes included -- gives the
oracle's panorama on thread-simulated ranks with the oracle as each rank's compute.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import pf_dist  # noqa: E402
import pf_layouts as PL  # noqa: E402
import pyoracle as O  # noqa: E402
import shard_shapes as S  # noqa: E402
import test_fuse_shapes as TS  # noqa: E402
from shard_sim import run_ranks  # noqa: E402
from test_dist import OracleRowBackend  # noqa: E402

CASE_IDS = [c["name"] for c in S.CASES]


def _layout_data(case):
    lay = S.LAYOUTS[case["layout"]]()
    tiles, total = O.make_tiles(lay)
    return lay, tiles, np.random.RandomState(3).rand(total).astype(np.float32)


@pytest.mark.parametrize("case", S.CASES, ids=CASE_IDS)
def test_row_is_what_it_is_for(case):
    lay, tiles, data = _layout_data(case)
    assert S.nlevels(case) == len(case["dims"]) == 3
    prev = None
    for lv, dims in enumerate(case["dims"]):
        L = S.level(case, lv)
        assert (L.w, L.h, L.h0, L.h1) == dims, f"level {lv}"
        if prev:
            assert (L.w, L.h) == (2 * prev[0], 2 * prev[1]), f"level {lv} does not double"
        prev = (L.w, L.h)
        assert 1 <= L.h0 < L.h1 <= L.h - 2, f"level {lv}"
        _, cnt, outside, clamped = O.targets(tiles, data, L)
        # no tap index leaves a tile's buffer in any row.  The edge layout's ranges are set in
        # whole columns of the finest level, so some of its taps lie a fraction of a pixel outside
        # their window (and read the tile's edge pixel); the other layouts have none of those
        assert clamped == 0, f"level {lv}"
        if case["layout"] == "edge":
            assert int((cnt >= 3).sum()) > 0 and int(cnt.max()) == 4, f"level {lv}"
            assert not cnt[:, 0].any() and not cnt[:, L.w - 1].any(), f"level {lv}"
        else:
            assert outside == 0 and int(cnt.max()) <= 2, f"level {lv}"
    assert case["dims"][-1][:2] == (case["out_w"], case["out_h"])
    eng = S.engines(case, tiles, data)
    assert tuple(lv for lv, (e, _) in enumerate(eng) if e == "sweeps") == case["sweeps"]
    if case["zr"] is S.ZR and case["layout"] != "edge":  # test_fuse_shapes' own rule agrees
        assert eng == TS.expected_engines(tiles, data, case["out_w"], case["out_h"])
    forms = {f for _, f in eng}
    if case["layout"] == "holes":
        assert forms == {"general"}
    # the worlds: the last rank of the largest world holds no tile, on C1 and the edge layout
    assert case["worlds"][:3] == (1, 2, 3)
    t0, t1 = pf_dist.shard_range(lay.ntiles, max(case["worlds"]) - 1, max(case["worlds"]))
    if max(case["worlds"]) > lay.ntiles:
        assert t0 == t1
    ew = case["baseline"][0]
    assert case["dims"][0][0] % ew != 0


def test_table_reaches_what_it_names():
    """The properties the issue lists, stated on the table itself."""
    by = S.BY_NAME
    d = {n: c["dims"] for n, c in by.items()}
    # the scalar border form (w % 4 = 2) and a partial patch column at every level
    assert d["c1-600x300"][0][0] % 4 == 2
    assert all(w % S.PATCH_W for w, _, _, _ in d["c1-600x300"])
    assert d["c1-360x180"][0][0] % S.PATCH_W == 26
    # band passes on 124 columns and below 128
    assert d["c1-496x248"][0][0] == 124 and d["c1-504x252"][0][0] == 126
    assert not by["c1-496x248"]["sweeps"] and not by["c1-504x252"]["sweeps"]
    # an odd-width level under the next level's upsample
    assert d["c1-500x248"][0][0] % 2 == 1 and by["c1-500x248"]["sweeps"] == (0,)
    # levels without band passes, one of them on the general form
    assert {n for n, c in by.items() if c["sweeps"]} == {"c1-500x248", "c1-440x220",
                                                         "c1-360x180"}
    # bands whose row count is no multiple of the patch height, odd first band rows
    odd = d["c1-512x256-odd"]
    assert all((h1 - h0 + 1) % S.PATCH_H for _, _, h0, h1 in odd)
    assert all(h0 % 2 == 1 for _, _, h0, _ in odd)
    # a row cut in the middle of a patch: [h0 + 3, h0 + 13) spans two patches of every band
    for c in S.CASES:
        for _, _, h0, h1 in c["dims"]:
            assert h1 - h0 + 1 > 13
    # heights other than width / 2
    assert all(by[n]["out_h"] != by[n]["out_w"] // 2 for n in ("c1-1096x500", "c1-1024x400"))
    # worlds without a tile for the last rank
    assert 7 in by["c1-600x300"]["worlds"] and 7 in by["c1-512x256-odd"]["worlds"]
    assert 9 in by["edge-512x256"]["worlds"]
    assert {c["layout"] for c in S.CASES} == {"c1", "holes", "edge"}
    assert {by[n]["layout"] for n in S.SIDE_CASES} == {"c1", "holes", "edge"}
    assert {c["baseline"] for c in S.CASES} == set(TS.BASELINES)


def test_500x250_is_no_size_the_fusion_takes():
    """Level 0 of 500x250 is 125x62 and level 1 is 250x125, not twice that: the oracle refuses the
    size (as pf_fuse does, tests/test_gpu_shard_shapes.py), so the table holds 500x248 for the
    125-wide level 0."""
    w, h = S.REFUSED_SIZE
    assert (O.level_dims(w, h, S.ZR, 0).w, O.level_dims(w, h, S.ZR, 0).h) == (125, 62)
    assert (O.level_dims(w, h, S.ZR, 1).w, O.level_dims(w, h, S.ZR, 1).h) == (250, 125)
    k = S.inputs("c1-500x248")
    with pytest.raises(ValueError, match=f"rc={O.ELEVELS}"):
        O.solve_depth_all(np.array(k["emap"]), k["tiles"], np.array(k["xdata"]), w, S.ZR, out_h=h)


def test_world2_bands_come_from_the_layout_world3_from_the_even_split():
    """C1 at world 2 deals one zenith band of tiles per rank, so the row bands start at the second
    rank's first tile row; at world 3 the tiles' first rows do not ascend with the rank."""
    case = S.BY_NAME["c1-600x300"]
    lay, tiles, data = _layout_data(case)
    for lv in range(3):
        L = S.level(case, lv)
        for world, dealt in ((2, True), (3, False)):
            ext = []
            for r in range(world):
                _, n = O.targets_subset(tiles, *pf_dist.shard_range(lay.ntiles, r, world), data, L)
                rows = np.nonzero(n.any(1))[0]
                ext.append((int(rows[0]), int(rows[-1])))
            even = pf_dist.band_bounds(L.h0, L.h1, world)
            got = pf_dist.band_bounds(L.h0, L.h1, world, ext, 1)
            assert (got != even) == dealt, (lv, world, got, even)
            if dealt:
                assert got[1] == ext[1][0]


class SweepsRowBackend(OracleRowBackend):
    """test_dist.OracleRowBackend whose plan() answers as pf_dist.HipRowShardBackend's: no band
    passes ([]) where the streamed engine does not take the level (test_fuse_shapes.tcap < 1)."""

    def plan(self, level, nbands):
        if TS.tcap(self._lv(level)) < 1:
            return []
        return super().plan(level, nbands)


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("name", ["c1-600x300", "c1-440x220"])
def test_row_sharded_orchestration_equals_oracle(name, world):
    """fuse_row_sharded on `world` threads, the oracle computing each rank's share: rank 0's u16
    equals the oracle's own fusion, bit for bit.  440x220: level 0 has no band passes, so the flow
    must replicate it although rep_levels is 0 -- at world 1 as well, where it asks for a plan it
    never uses.  The bytes each rank sends are those of exchange_model under the same rule."""
    k = S.inputs(name)
    case = k["case"]
    assert case["out_h"] == case["out_w"] // 2 and case["zr"] is S.ZR  # OracleBackend's
    ref = S.reference(name)
    nt = k["lay"].ntiles
    emap = np.array(k["emap"])

    def body(r, comm):
        be = SweepsRowBackend(O, PL, case["out_w"], emap, k["tiles"], np.array(k["xdata"]))
        log = pf_dist.ExchangeLog()
        pf_dist.fuse_row_sharded(be, 3, nt, r, world, comm, log, rep_levels=0)
        dims = [be.dims(lv) for lv in range(3)]
        plans = [be.plan(lv, world) for lv in range(3)]
        ext = [[be.tile_rows(lv, *pf_dist.shard_range(nt, q, world)) for q in range(world)]
               for lv in range(3)]
        model = pf_dist.exchange_model(dims, plans, ext, world, rep_levels=0)[r]
        assert all(model.get(key, 0) == v for key, v in log.sent.items()) and \
            all(log.sent.get(key, 0) == v for key, v in model.items()), (r, model, log.sent)
        assert pf_dist.auto_rep_levels(be, 3, world) >= (len(case["sweeps"]) if world > 1 else 0)
        return be.out.numpy().view(np.uint16).reshape(case["out_h"], case["out_w"])

    outs, errs = run_ranks(world, body)
    assert not any(errs), errs
    bad = int((outs[0] != ref).sum())
    assert bad == 0, f"{name} world {world}: {bad} pixels differ from the oracle"
    assert np.count_nonzero(ref) > case["out_w"]


def test_level_without_band_passes_after_a_sharded_level_is_refused():
    """Such a level cannot be replicated once a level before it is row-sharded (every rank would
    need that whole level): a ValueError on every rank, before any exchange."""
    k = S.inputs("c1-600x300")
    case = k["case"]

    class Backend(OracleRowBackend):
        def plan(self, level, nbands):
            return [] if level == 1 else super().plan(level, nbands)

    logs = [pf_dist.ExchangeLog() for _ in range(2)]

    def body(r, comm):
        be = Backend(O, PL, case["out_w"], np.array(k["emap"]), k["tiles"], np.array(k["xdata"]))
        pf_dist.fuse_row_sharded(be, 3, k["lay"].ntiles, r, 2, comm, logs[r])

    _, errs = run_ranks(2, body)
    assert all(isinstance(e, ValueError) and "no band passes" in str(e) for e in errs), errs
    assert all(not log.sent and log.rounds == 0 for log in logs)
    with pytest.raises(ValueError, match="no band passes"):
        pf_dist.exchange_model([(8, 40, 4, 35)] * 3, [[2], [], [2]], [[(5, 34)] * 2] * 3, 2)
