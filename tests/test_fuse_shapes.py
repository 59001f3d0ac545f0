"""The fusion's shape table: output sizes that are not powers of two, checked on the CPU.

SHAPES is the table tests/test_gpu_fuse_shapes.py fuses on the GPU.  Each row names an output
size, the dims and band of its three levels and the Jacobi engine each level takes with the C1
layout.  Nothing in a row is assumed: the dims and bands are compared with the oracle's
(pfo_level_dims), the oracle's targets must see no out-of-tile tap and no pixel covered more than
twice, and the engine column must follow from expected_engines(), a restatement of the host's
rules on the oracle's coverage counts:

* certificate (prepare_levels, csrc/pf_layout.hip): the coverage is separable -- a band pixel is
  covered iff its row is in h0+1..h1-1 and its column is in the covered set of row h0+1 -- and
  column 0 is uncovered.  With it a level takes the packed form, without it the general form.
* sweeps (fuse_range, csrc/pf_fuse.hip): jacobi_tcap(L) < 1, with tcap = min(10, h0-1, h-2-h1),
  lowered until 128 - 4*ceil(tcap/4) <= w and w is even.
* resident (jres_plan, csrc/pf_plan.hip): otherwise, if the level has the certificate, w is 256
  or 512 and some blocking of the band fits the kernel's region rows.  The host asks this at every
  level, not only at level 0: a 1024-wide output has a resident 256-wide level 0 and a resident
  512-wide level 1.
* streamed: otherwise.

What each row is for:
  600x300    w % 4 = 2 at level 0 (the scalar border kernel), w % 64 != 0 at every level (partial
             target patches), ragged last strips, odd level-0 height
  496x248    124: the narrowest width the streamed engine accepts, a strip wider than a row
  504x252    w < 128, odd level-0 height
  500x248    odd level-0 width (sweeps), then the streamed upsample of an odd-width level
  440x220    narrow level 0 without the certificate, then packed
  360x180    narrow, w % 64 = 26
  1096x500   height != width / 2
  1024x400   the 256-wide resident instantiation at level 0 (band 73 rows), 512-wide at level 1
  1024x640   band 115 rows: fits one 128-row region
  1024x1000  band 179 rows > 128: the plan must split the panorama into row blocks
  2048x400   the 512-wide instantiation at level 0 with a 73-row band (64- / 32-row regions)
"""
import numpy as np
import pytest

import pf_layouts as PL
import pyoracle as O

ZR = PL.ZENITH_RANGE

# (out_w, out_h, ((w, h, h0, h1), ...) per level, (engine, ...) per level)
SHAPES = [
    (600, 300, ((150, 75, 10, 65), (300, 150, 21, 129), (600, 300, 43, 257)),
     ("streamed", "streamed", "streamed")),
    (496, 248, ((124, 62, 8, 54), (248, 124, 17, 107), (496, 248, 35, 213)),
     ("streamed", "streamed", "streamed")),
    (504, 252, ((126, 63, 9, 54), (252, 126, 18, 108), (504, 252, 36, 216)),
     ("streamed", "streamed", "streamed")),
    (500, 248, ((125, 62, 8, 54), (250, 124, 17, 107), (500, 248, 35, 213)),
     ("sweeps", "streamed", "streamed")),
    (440, 220, ((110, 55, 7, 48), (220, 110, 15, 95), (440, 220, 31, 189)),
     ("sweeps", "streamed", "streamed")),
    (360, 180, ((90, 45, 6, 39), (180, 90, 12, 77), (360, 180, 25, 154)),
     ("sweeps", "streamed", "streamed")),
    (1096, 500, ((274, 125, 18, 107), (548, 250, 36, 214), (1096, 500, 72, 428)),
     ("streamed", "streamed", "streamed")),
    (1024, 400, ((256, 100, 14, 86), (512, 200, 28, 172), (1024, 400, 57, 343)),
     ("resident", "resident", "streamed")),
    (1024, 640, ((256, 160, 23, 137), (512, 320, 46, 274), (1024, 640, 92, 548)),
     ("resident", "resident", "streamed")),
    (1024, 1000, ((256, 250, 36, 214), (512, 500, 72, 428), (1024, 1000, 144, 856)),
     ("resident", "resident", "streamed")),
    (2048, 400, ((512, 100, 14, 86), (1024, 200, 28, 172), (2048, 400, 57, 343)),
     ("resident", "streamed", "streamed")),
]
# levels of SHAPES without the certificate (the general form): level 0 of 440x220, which takes
# the per-sweep kernel anyway
NO_CERTIFICATE = {(440, 220, 0)}
# the rows whose level 0 is resident, and those where no single row block holds the band
RESIDENT_ROWS = [(1024, 400), (1024, 640), (1024, 1000), (2048, 400)]
SPLIT_ROWS = [(1024, 1000), (2048, 400)]

# baselines that do not divide a level-0 width: (ew, eh, channels), row i takes BASELINES[i % 3]
BASELINES = [(100, 50, 1), (77, 31, 1), (96, 40, 3)]

# the coverage-hole case: C1 without this tile, at HOLES_SHAPE
HOLES_SHAPE = (600, 300)
HOLES_DROP = 4


def shape_id(row):
    return f"{row[0]}x{row[1]}"


def holes_layout():
    """C1 with one mid-band tile dropped: uncovered band pixels, so no level has the certificate."""
    full = PL.config_layout("C1")
    keep = [i for i in range(full.ntiles) if i != HOLES_DROP]
    return PL.Layout("C1-holes", full.fovs[keep], full.ranges[keep], full.tile_w[keep],
                     full.tile_h[keep])


def has_certificate(cnt, lv):
    cov = cnt > 0
    if not lv.h0 + 1 < lv.h1:
        return False
    cols = cov[lv.h0 + 1]
    if cols[0]:
        return False
    rows = np.zeros(lv.h, bool)
    rows[lv.h0 + 1:lv.h1] = True
    band = slice(lv.h0, lv.h1 + 1)
    return bool(np.array_equal(cov[band], (rows[:, None] & cols[None, :])[band]))


def tcap(lv):
    cap = min(10, lv.h0 - 1, lv.h - 2 - lv.h1)
    while cap >= 1 and not (128 - 4 * ((cap + 3) // 4) <= lv.w and lv.w % 2 == 0):
        cap -= 1
    return cap


def resident_blockings(lv):
    """The row blockings jres_plan may choose for a level: [(region rows, nb, core, K)]."""
    regions = {512: (64, 32), 256: (128,)}.get(lv.w, ())
    band = lv.h1 - lv.h0 + 1
    plans = []
    for rows in regions:
        for nb in range(1, min(band, 64) + 1):
            core = -(-band // nb)
            if -(-band // core) != nb:
                continue
            if nb == 1:
                if core > rows:
                    continue
                k = lv.iters
            else:
                k = min((rows - core) // 2, core, lv.iters)
                if k < 1:
                    continue
            plans.append((rows, nb, core, k))
    return plans


def expected_engines(tiles, data, out_w, out_h, certificate=None):
    """[(engine, form)] per level for a layout's oracle tiles: the host's rules restated.
    certificate=False: under the tile validity rule, where level_full() answers false."""
    res = []
    for level in range(O.num_levels(out_w)):
        lv = O.level_dims(out_w, out_h, ZR, level)
        _, cnt, oops, _ = O.targets(tiles, data, lv)
        assert oops == 0
        cert = has_certificate(cnt, lv) if certificate is None else bool(certificate)
        if tcap(lv) < 1:
            engine = "sweeps"
        elif cert and resident_blockings(lv):
            engine = "resident"
        else:
            engine = "streamed"
        res.append((engine, "packed" if cert else "general"))
    return res


@pytest.fixture(scope="module")
def c1():
    tiles, total = O.make_tiles(PL.config_layout("C1"))
    return tiles, np.random.RandomState(3).rand(total).astype(np.float32)


@pytest.mark.parametrize("row", SHAPES, ids=shape_id)
def test_shape_row(c1, row):
    out_w, out_h, dims, engines = row
    tiles, data = c1
    assert O.num_levels(out_w) == len(dims) == len(engines) == 3
    prev = None
    for level, (w, h, h0, h1) in enumerate(dims):
        lv = O.level_dims(out_w, out_h, ZR, level)
        assert (lv.w, lv.h, lv.h0, lv.h1) == (w, h, h0, h1), f"level {level}"
        if prev:
            assert (w, h) == (2 * prev[0], 2 * prev[1]), f"level {level} does not double"
        prev = (w, h)
        # the band prepare_levels accepts
        assert 1 <= h0 and h1 <= h - 2 and h0 < h1, f"level {level}"
        _, cnt, oops, _ = O.targets(tiles, data, lv)
        assert oops == 0, f"level {level}: {oops} taps outside their tile"
        assert int(cnt.max()) <= 2, f"level {level}: coverage {int(cnt.max())}"
    assert dims[-1][:2] == (out_w, out_h)
    got = expected_engines(tiles, data, out_w, out_h)
    assert tuple(e for e, _ in got) == engines
    for level, (_, form) in enumerate(got):
        want = "general" if (out_w, out_h, level) in NO_CERTIFICATE else "packed"
        assert form == want, f"level {level}"


def test_table_reaches_what_it_names(c1):
    """The properties the rows were chosen for, stated on the table itself."""
    rows = {(r[0], r[1]): r for r in SHAPES}
    lv0 = {k: r[2][0] for k, r in rows.items()}
    assert lv0[(600, 300)][0] % 4 == 2 and all(d[0] % 64 for d in rows[(600, 300)][2])
    assert lv0[(496, 248)][0] == 124 and lv0[(504, 252)][0] < 128 and lv0[(504, 252)][1] % 2
    assert lv0[(500, 248)][0] % 2 == 1 and rows[(500, 248)][3][1] == "streamed"
    assert lv0[(360, 180)][0] % 64 == 26
    assert rows[(1096, 500)][1] != rows[(1096, 500)][0] // 2
    engines = {e for r in SHAPES for e in r[3]}
    assert engines == {"resident", "streamed", "sweeps"}
    # both resident widths at level 0, and the blockings of the rows that must split
    assert {lv0[k][0] for k in RESIDENT_ROWS} == {256, 512}
    for k in RESIDENT_ROWS:
        assert rows[k][3][0] == "resident"
        lv = O.level_dims(k[0], k[1], ZR, 0)
        nbs = {p[1] for p in resident_blockings(lv)}
        assert nbs, k
        assert (min(nbs) >= 2) == (k in SPLIT_ROWS), (k, sorted(nbs))
    # 1024x640 may be forced to 2 and 3 row blocks
    lv = O.level_dims(1024, 640, ZR, 0)
    assert {1, 2, 3} <= {p[1] for p in resident_blockings(lv)}


def test_holes_layout_has_no_certificate():
    lay = holes_layout()
    tiles, total = O.make_tiles(lay)
    data = np.random.RandomState(4).rand(total).astype(np.float32)
    got = expected_engines(tiles, data, *HOLES_SHAPE)
    assert got == [("streamed", "general")] * 3
    for level in range(3):
        lv = O.level_dims(*HOLES_SHAPE, ZR, level)
        _, cnt, _, _ = O.targets(tiles, data, lv)
        inner = cnt[lv.h0 + 1:lv.h1]
        assert int((inner[:, 1:] == 0).sum()) > 0 and int(cnt.max()) <= 2


@pytest.mark.parametrize("i", range(len(BASELINES)))
def test_baselines_do_not_divide_level0(c1, i):
    """The rotated baselines leave every level-0 width undivided, and the oracle fuses them."""
    ew, eh, ec = BASELINES[i]
    for k, row in enumerate(SHAPES):
        if k % len(BASELINES) == i:
            assert row[2][0][0] % ew != 0, shape_id(row)
    tiles, data = c1
    emap = np.random.RandomState(5 + i).rand(*((eh, ew) if ec == 1 else (eh, ew, ec)))
    out, oops = O.solve_depth_all(emap.astype(np.float32), tiles, data, 600, ZR, out_h=300)
    assert out.shape == (300, 600) and oops == 0 and np.count_nonzero(out) > 0


def test_oracle_refuses_band_at_a_pole(c1):
    """A band that reaches the last row (level 0 of 440x220 at 3..177 degrees: h1 = h - 1) made the
    oracle write past its buffers; it is refused before any buffer is touched.  The wide band the
    GPU accepts, 1024x512 at the same range, still runs."""
    zr = (np.float32(PL.D2R(3.0)), np.float32(PL.D2R(177.0)))
    lv = O.level_dims(440, 220, zr, 0)
    assert lv.h1 > lv.h - 2
    tiles, data = c1
    emap = np.random.RandomState(6).rand(50, 100).astype(np.float32)
    with pytest.raises(ValueError, match=f"rc={O.EBAND}"):
        O.solve_depth_all(emap, tiles, data, 440, zr, out_h=220)
    for level in range(3):
        lv = O.level_dims(1024, 512, zr, level)
        assert 1 <= lv.h0 < lv.h1 <= lv.h - 2
    lay = PL.band_layout(5, 4, 256, 256, 3, 12, "wide", z_lo=4.0, z_hi=176.0)
    wt, total = O.make_tiles(lay)
    wd = np.random.RandomState(11).rand(total).astype(np.float32)
    out, _ = O.solve_depth_all(emap, wt, wd, 1024, zr)
    assert out.shape == (512, 1024) and np.count_nonzero(out) > 0
