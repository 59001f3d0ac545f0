"""The fusion at output sizes that are not powers of two, against the CPU oracle.

Every other fusion test runs at widths 512..8192 with height = width / 2 and a baseline whose
width divides the level-0 width.  The rows of test_fuse_shapes.SHAPES (checked there on the CPU)
reach what those sizes never do: ragged last strips and strips wider than a row in the streamed
Jacobi passes, the per-sweep kernels taken for a width reason, an odd-width level under the
streamed upsample, the scalar border kernel, partial 64x8 target patches, the 256-wide resident
kernel at level 0 and both resident widths at bands other than C2's, and seed tables for baselines
that do not divide the level width (one and three channels).

Inputs are the C1 layout's tiles warped from a 512x256 synthetic scene; the reference is
pyoracle.solve_depth_all(..., out_h=h).  Every comparison is array_equal on u16 or on fp32 bit
patterns.  PF_JPLAN is read once per process, so one fresh child process fuses every case with
PF_JPLAN=1: its `jacobi plan` lines must name the engine test_fuse_shapes expects for every level
of every case, and its outputs must equal the oracle's too.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import panofuse  # noqa: E402
import pf_layouts as PL  # noqa: E402
import pf_synth  # noqa: E402
import pyoracle as O  # noqa: E402
import test_fuse_shapes as TS  # noqa: E402
from test_fuse_shapes import BASELINES, RESIDENT_ROWS, SHAPES, SPLIT_ROWS, shape_id  # noqa: E402

ZR = PL.ZENITH_RANGE
DEV = "cuda:0"
SEED = 20261020
ROW = {(r[0], r[1]): i for i, r in enumerate(SHAPES)}
BATCH_ROWS = [(600, 300), (1024, 400)]
NBATCH = 9  # one more than the targets kernel's 8 panoramas per block
SWEEPS_LEVEL = (500, 248)  # its level 0 (125 wide) takes the per-sweep form in pf_fuse_level too


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _tile_data(lay, n, base):
    """(oracle tiles, float32 [n, tile_elems]): the layout's tiles of n synthetic 512x256 scenes."""
    tiles, total = O.make_tiles(lay)
    seeds = pf_synth.seeds_for(n, base)
    gt = pf_synth.scene_depth(seeds, 512, 256).numpy()
    resp = pf_synth.responses(seeds, lay.ntiles)
    nt = lay.ntiles
    data = np.stack([O.warp_depth(gt[b], tiles, total, O.responses(resp[b * nt:(b + 1) * nt]))
                     for b in range(n)])
    return tiles, data


def _emaps(n, base, ew, eh, ec):
    """float32 [n, eh, ew] or [n, eh, ew, ec] baselines; the channels past the first are noise."""
    e = pf_synth.baseline_emap(pf_synth.seeds_for(n, base), ew, eh).numpy().astype(np.float32)
    if ec == 1:
        return np.ascontiguousarray(e)
    rest = np.random.RandomState(base % (1 << 31)).rand(n, eh, ew, ec - 1).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([e[..., None], rest], -1))


def _inputs():
    """The inputs of every case, the same in the parent and the child: no oracle fusion here."""
    c1 = PL.config_layout("C1")
    holes = TS.holes_layout()
    tiles_c1, data_c1 = _tile_data(c1, 1, SEED)
    tiles_h, data_h = _tile_data(holes, 1, SEED + 1)
    emaps = [_emaps(1, SEED + 10 + i, *BASELINES[i % len(BASELINES)])[0]
             for i in range(len(SHAPES))]
    return {"c1": (c1, tiles_c1, data_c1[0]), "holes": (holes, tiles_h, data_h[0]),
            "emaps": emaps}


def _jobs():
    """The child's fusions: (layout key, row index, resident or None = the default, row_blocks)."""
    jobs = [("c1", i, None, 0) for i in range(len(SHAPES))]
    jobs.append(("holes", ROW[TS.HOLES_SHAPE], None, 0))
    jobs += [("c1", ROW[(1024, 640)], True, nb) for nb in (2, 3)]
    jobs += [("c1", ROW[k], False, 0) for k in RESIDENT_ROWS]
    return jobs


def _fuse(f, emap, data, out_w, out_h):
    out = torch.zeros((1, out_h, out_w), dtype=torch.int16, device=DEV)
    f.fuse(_dev(emap)[None], _dev(data)[None].contiguous(), out, ZR)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint16)[0]


def _child(out_path):
    inp = _inputs()
    outs, errs = {}, []
    for k, (key, i, resident, nb) in enumerate(_jobs()):
        lay, _, data = inp[key]
        f = panofuse.Fuser(0)
        try:
            f.set_tiles(lay)
            if resident is not None:
                f.set_jacobi_engine(resident=resident, row_blocks=nb)
            outs[f"out{k}"] = _fuse(f, inp["emaps"][i], data, SHAPES[i][0], SHAPES[i][1])
            errs.append(f.jres_errors())
        finally:
            f.close()
    # pf_fuse_level's per-sweep branch prints a plan line of its own: the last line of this run
    w, h = SWEEPS_LEVEL
    lay, _, data = inp["c1"]
    lv = O.level_dims(w, h, ZR, 0)
    f = panofuse.Fuser(0)
    try:
        f.set_tiles(lay)
        lsum = torch.zeros(lv.h * lv.w, dtype=torch.float32, device=DEV)
        cnt, buf = torch.zeros_like(lsum), torch.zeros_like(lsum)
        f.fuse_partial(_dev(data), None, 0, lay.ntiles, w, ZR, 0, lsum, cnt, out_h=h)
        f.fuse_level(_dev(inp["emaps"][ROW[SWEEPS_LEVEL]])[None], None, lsum, cnt, w, ZR, 0, buf,
                     out_h=h)
        torch.cuda.synchronize()
        outs["level0"] = buf.cpu().numpy().reshape(lv.h, lv.w)
    finally:
        f.close()
    np.savez(out_path, errs=np.array(errs, np.int64), **outs)


CHILD = ("import sys; sys.path[:0] = [{pkg!r}, {oracle!r}, {tests!r}]; "
         "import test_gpu_fuse_shapes as t; t._child(sys.argv[1])")
PLAN = re.compile(r"^jacobi plan (\d+)x(\d+) band (\d+) iters (\d+) batch (\d+) (.*)$")


@pytest.fixture(scope="module")
def fuser():
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected on a host without a GPU")
    f = panofuse.Fuser(0)
    f.set_tiles(PL.config_layout("C1"))
    return f


@pytest.fixture(scope="module")
def inputs():
    return _inputs()


@pytest.fixture(scope="module")
def refs(inputs):
    """The oracle's u16 panorama of every table row (C1), computed once."""
    _, tiles, data = inputs["c1"]
    res = []
    for i, (w, h, _, _) in enumerate(SHAPES):
        ref, oops = O.solve_depth_all(inputs["emaps"][i], tiles, data, w, ZR, out_h=h)
        assert oops == 0 and ref.shape == (h, w)
        res.append(ref)
    return res


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    """One child process with PF_JPLAN=1 over _jobs(): ([u16 panorama], [jres errors], [[plan
    line fields per level]])."""
    out_path = tmp_path_factory.mktemp("shapes") / "child.npz"
    here = os.path.dirname(os.path.abspath(__file__))
    code = CHILD.format(pkg=os.path.dirname(os.path.abspath(panofuse.__file__)),
                        oracle=os.path.dirname(os.path.abspath(O.__file__)), tests=here)
    env = dict(os.environ, PF_JPLAN="1")
    for k in ("PF_JSLOW", "PF_JRES", "PF_JACOBI", "PF_JRES_NB"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", code, str(out_path)], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    plans = [PLAN.match(ln).groups() for ln in r.stderr.splitlines()
             if ln.startswith("jacobi plan")]
    jobs = _jobs()
    assert len(plans) == 3 * len(jobs) + 1, r.stderr[-3000:]
    z = np.load(out_path)
    return ([z[f"out{k}"] for k in range(len(jobs))], z["errs"].tolist(),
            [plans[3 * k:3 * k + 3] for k in range(len(jobs))], plans[-1], z["level0"])


def _diff(got, ref):
    assert got.shape == ref.shape and got.dtype == ref.dtype == np.uint16
    return int((got != ref).sum())


# ---- a. whole fusion, every row ---------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=[shape_id(r) for r in SHAPES])
def test_fuse_matches_oracle(fuser, inputs, refs, i):
    w, h = SHAPES[i][:2]
    got = _fuse(fuser, inputs["emaps"][i], inputs["c1"][2], w, h)
    bad = _diff(got, refs[i])
    assert bad == 0, f"{w}x{h}: {bad} of {got.size} pixels differ from the oracle"
    assert np.count_nonzero(got) > 0
    assert fuser.jres_errors() == 0


# ---- b, f. the engine of every level, from the child's plan lines -----------------------------
def _expected_lines(inputs, key, i, resident, nb):
    """[(w, h, band, iters, engine, form)] per level of a child job (test_fuse_shapes' rules)."""
    _, tiles, data = inputs[key]
    out_w, out_h = SHAPES[i][:2]
    exp = []
    for level, (engine, form) in enumerate(TS.expected_engines(tiles, data, out_w, out_h)):
        lv = O.level_dims(out_w, out_h, ZR, level)
        if engine == "resident":
            if resident is False:
                engine = "streamed"
            elif nb and not any(p[1] == nb for p in TS.resident_blockings(lv)):
                engine = "streamed"  # no blocking of that many row blocks fits: streamed passes
        exp.append((lv.w, lv.h, lv.h1 - lv.h0 + 1, lv.iters, engine, form))
    return exp


def test_child_engines_and_outputs(inputs, refs, child):
    outs, errs, plans, _, _ = child
    _, tiles_h, data_h = inputs["holes"]
    hi = ROW[TS.HOLES_SHAPE]
    ref_holes, oops = O.solve_depth_all(inputs["emaps"][hi], tiles_h, data_h, SHAPES[hi][0], ZR,
                                        out_h=SHAPES[hi][1])
    assert oops == 0
    seen = set()
    for k, (key, i, resident, nb) in enumerate(_jobs()):
        tag = f"job {k} ({key} {shape_id(SHAPES[i])} resident={resident} row_blocks={nb})"
        exp = _expected_lines(inputs, key, i, resident, nb)
        for level, (line, e) in enumerate(zip(plans[k], exp)):
            w, h, band, iters, batch, rest = line
            assert (int(w), int(h), int(band), int(iters), int(batch)) == e[:4] + (1,), (tag, line)
            engine, form = e[4], e[5]
            if engine == "resident":
                assert rest.startswith("resident: nb "), (tag, level, line)
                if nb:
                    assert rest.startswith(f"resident: nb {nb} "), (tag, level, line)
                seen.add(("resident", int(w)))
            elif engine == "streamed":
                assert rest.startswith(f"{form} C"), (tag, level, line)
                seen.add((form, 0))
            else:
                assert rest == "sweeps", (tag, level, line)
                seen.add(("sweeps", 0))
        if key == "c1" and resident is None:
            assert tuple(e[4] for e in exp) == SHAPES[i][3], tag
        ref = ref_holes if key == "holes" else refs[i]
        bad = _diff(outs[k], ref)
        assert bad == 0, f"{tag}: {bad} pixels differ from the oracle"
        assert errs[k] == 0, tag
    # all three engines, both forms of the streamed one, both resident widths
    assert seen >= {("resident", 256), ("resident", 512), ("packed", 0), ("general", 0),
                    ("sweeps", 0)}
    # the holes layout: the general form at every level
    k = [j[0] for j in _jobs()].index("holes")
    assert all(ln[5].startswith("general C") for ln in plans[k]), plans[k]


def test_child_fuse_level_sweeps_line(inputs, child):
    """pf_fuse_level at a level the streamed engine refuses: the per-sweep form, named by its own
    plan line, equal to the oracle's level."""
    _, _, _, line, got = child
    w, h = SWEEPS_LEVEL
    lv = O.level_dims(w, h, ZR, 0)
    assert TS.tcap(lv) < 1
    assert line == (str(lv.w), str(lv.h), str(lv.h1 - lv.h0 + 1), str(lv.iters), "1", "sweeps")
    _, tiles, data = inputs["c1"]
    rL, rn, _, _ = O.targets(tiles, data, lv)
    ref = O.jacobi(O.seed_level0(inputs["emaps"][ROW[SWEEPS_LEVEL]], lv), O.normalize(rL, rn, lv),
                   lv, lv.iters)
    assert got.shape == ref.shape
    assert int((_bits(got) != _bits(ref)).sum()) == 0


# ---- c. resident against streamed --------------------------------------------------------------
@pytest.mark.parametrize("shape", RESIDENT_ROWS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_resident_equals_streamed(inputs, refs, child, shape):
    i = ROW[shape]
    lay, _, data = inputs["c1"]
    engines = [(True, 0), (False, 0)]
    if shape == (1024, 640):
        engines += [(True, 2), (True, 3)]  # hand-offs where the plan takes one block
    got = {}
    for resident, nb in engines:
        f = panofuse.Fuser(0)
        try:
            f.set_tiles(lay)
            f.set_jacobi_engine(resident=resident, row_blocks=nb)
            got[(resident, nb)] = _fuse(f, inputs["emaps"][i], data, shape[0], shape[1])
            assert f.jres_errors() == 0, (resident, nb)
        finally:
            f.close()
    for key, out in got.items():
        bad = _diff(out, refs[i])
        assert bad == 0, f"{shape} resident={key[0]} row_blocks={key[1]}: {bad} pixels differ"
    assert np.array_equal(got[(True, 0)], got[(False, 0)])
    # what ran in this process, from the child's plan lines of the same settings
    _, _, plans, _, _ = child
    jobs = _jobs()
    line0 = plans[jobs.index(("c1", i, None, 0))][0][5]
    assert line0.startswith("resident: nb "), line0
    nb0 = int(line0.split()[2])
    if shape in SPLIT_ROWS:
        assert nb0 >= 2, line0
    assert plans[jobs.index(("c1", i, False, 0))][0][5].startswith("packed C")
    if shape == (1024, 640):
        assert nb0 == 1, line0
        for nb in (2, 3):
            ln = plans[jobs.index(("c1", i, True, nb))][0][5]
            assert ln.startswith(f"resident: nb {nb} "), ln


# ---- d. batches --------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", BATCH_ROWS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_batches(fuser, shape):
    """Batches 3 and 9 of distinct panoramas and baselines: every panorama equals its own batch-1
    fusion, and panorama 0 and the last of each batch equal the oracle."""
    i = ROW[shape]
    w, h = shape
    lay = PL.config_layout("C1")
    tiles, datas = _tile_data(lay, NBATCH, SEED + 100 + i)
    emaps = _emaps(NBATCH, SEED + 200 + i, *BASELINES[i % len(BASELINES)])
    single = [_fuse(fuser, emaps[b], datas[b], w, h) for b in range(NBATCH)]
    for b in sorted({0, 2, NBATCH - 1}):
        ref, _ = O.solve_depth_all(emaps[b], tiles, datas[b], w, ZR, out_h=h)
        bad = _diff(single[b], ref)
        assert bad == 0, f"{shape} panorama {b}: {bad} pixels differ from the oracle"
    assert not np.array_equal(single[0], single[1])
    for B in (3, NBATCH):
        out = torch.zeros((B, h, w), dtype=torch.int16, device=DEV)
        fuser.fuse(_dev(emaps[:B]), _dev(datas[:B]), out, ZR)
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(np.uint16)
        for b in range(B):
            bad = _diff(got[b], single[b])
            assert bad == 0, f"{shape} batch {B} panorama {b}: {bad} pixels differ from batch 1"
    assert fuser.jres_errors() == 0


# ---- e. level internals ------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("shape", [(600, 300), (500, 248)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_level_internals(fuser, inputs, shape):
    """Seed / upsample planes, coverage counts and summed targets inside the band, the Jacobi
    result of every level, and the tap-index maps: through fuse_seed + fuse_partial +
    fuse_finish_level, and once more through fuse_level."""
    out_w, out_h = shape
    i = ROW[shape]
    lay, tiles, data = inputs["c1"]
    emap = inputs["emaps"][i]
    t_tiles, t_emap = _dev(data), _dev(emap)[None]
    prev_a = prev_b = prev_ref = None
    for level in range(O.num_levels(out_w)):
        lv = O.level_dims(out_w, out_h, ZR, level)
        taps = fuser.probe_taps(out_w, ZR, level, out_h=out_h).cpu().numpy()
        ref_taps = O.probe_taps(tiles, lv)
        assert taps.shape == ref_taps.shape
        assert int((taps != ref_taps).sum()) == 0, f"taps L{level}"

        buf = torch.zeros(lv.h * lv.w, dtype=torch.float32, device=DEV)
        fuser.fuse_seed(t_emap if level == 0 else None, prev_a, out_w, ZR, level, buf,
                        out_h=out_h)
        ref_seed = O.seed_level0(emap, lv) if level == 0 else O.upsample(prev_ref, lv)
        assert np.array_equal(_bits(buf.cpu().numpy().reshape(lv.h, lv.w)), _bits(ref_seed)), \
            f"seed L{level}"
        lsum = torch.zeros(lv.h * lv.w, dtype=torch.float32, device=DEV)
        cnt = torch.zeros_like(lsum)
        fuser.fuse_partial(t_tiles, None, 0, lay.ntiles, out_w, ZR, level, lsum, cnt, out_h=out_h)
        rL, rn, oops, _ = O.targets(tiles, data, lv)
        assert oops == 0
        band = slice(lv.h0, lv.h1 + 1)
        g_l = lsum.cpu().numpy().reshape(lv.h, lv.w)[band]
        g_n = cnt.cpu().numpy().reshape(lv.h, lv.w)[band]
        assert np.array_equal(g_n, rn[band].astype(np.float32)), f"coverage L{level}"
        assert np.array_equal(_bits(g_l), _bits(rL[band])), f"targets L{level}"
        ref_buf = O.jacobi(ref_seed, O.normalize(rL, rn, lv), lv, lv.iters)

        fuser.fuse_finish_level(lsum, cnt, out_w, ZR, level, buf, out_h=out_h)
        got = buf.cpu().numpy().reshape(lv.h, lv.w)
        bad = int((_bits(got) != _bits(ref_buf)).sum())
        assert bad == 0, f"{shape} level {level}: {bad} Jacobi values differ (fuse_finish_level)"

        buf_b = torch.zeros(lv.h * lv.w, dtype=torch.float32, device=DEV)
        fuser.fuse_level(t_emap if level == 0 else None, prev_b, lsum, cnt, out_w, ZR, level,
                         buf_b, out_h=out_h)
        got = buf_b.cpu().numpy().reshape(lv.h, lv.w)
        bad = int((_bits(got) != _bits(ref_buf)).sum())
        assert bad == 0, f"{shape} level {level}: {bad} Jacobi values differ (fuse_level)"
        prev_a, prev_b, prev_ref = buf, buf_b, ref_buf
    assert fuser.jres_errors() == 0
