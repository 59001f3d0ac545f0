"""The load schedule of the streamed Jacobi passes (k_jlag): L rows are loaded straight into their
ring slot LL steps ahead and sanitised there, input rows land in NB buffers indexed by ring group
plus phase, and the drain rotates both to ring group 0.

C1 (512 x 256, levels of width 128 / 256 / 512 with bands of 47 / 93 / 185 rows), three panoramas,
the streaming engine forced so that level 0 takes the seeded first pass too.  Every case forces a
sweep depth (PF_JT<w>, PF_JTONLY<w>) and a row chunking (PF_JN<w>) and compares, exactly,
  * every level's float plane of every panorama (pf_fuse_level, one panorama per call: the seeded
    and the upsampling first passes, the float stores) with the oracle's Jacobi of that level, and
  * the batched fusion's u16 panoramas (pf_fuse: blockIdx.y = panorama, the u16 stores) with the
    oracle's SolveDepthAll.
The oracle's planes are computed once per module.  The planner reads its engine switches once per
process, so the cases run in one fresh child process with the pipelined engine off (PF_JPIPE=0:
every pass is a k_jlag launch) and its plan lines (PF_JPLAN) must show the forced depth and chunks.

Level 0's band leaves room for depths up to 7 (jacobi_tcap), so depths 8 and 10 run on levels 1
and 2 while level 0 runs depth 5.

What the chunk lengths are for (a chunk of r rows runs r + 3T + 1 steps in gt = ceil(steps / 6)
groups; the fill is NF groups, the drain ND = 1 group starting in ring group (gt - 1) % NG):
  * T = 10 (R = 24, NG = 4, LL = 3, NB = 4): gt >= 6 > NF + ND = 4 for every r >= 1, so the
    fill's early return and the drain-less loop cannot be reached at this depth, and neither at
    T = 8 (gt >= 5 = NF + ND).  r = 1 and r = LL = 3 (drain group 1), r in 6..11 (group 2), 12..17
    (group 3), 18..23 (group 0): the four rotation shifts and both input-buffer phases.
  * T = 8 (R = 18, NG = 3, LL = 1, NB = 3): r = 1 = LL (group 1), 6..11 (group 2), 12..17 (group 0).
  * T = 4 (R = 12, NF = 3): r <= 5 ends inside the fill (gt = 3 = NF + ND - 1: the early return,
    no drain), r = 6 is exactly NF + ND groups (drain taken).  T = 5: r <= 2 and r = 3 likewise.
  * T = 1 and T = 2 (R = 6, NG = 1): no rotation; r = 2 at T = 1 is one group (early return).

A non-finite target on covered pixels: panorama 1's tile 0 holds +inf in one pixel (INF_PIXEL),
in every case.  The levels sample a tile by nearest pixel; the pixel is chosen so that no 5-point
stencil of any level takes it twice with opposite signs (inf - inf: a NaN would spread over the
oracle's whole band), which the fixture asserts.  At levels 0 and 2 one covered pixel then has
L = +inf (the stencil's centre) and four have L = -inf (a neighbour tap); the reference saturates
them to 1 and 0, and the oracle's planes stay finite everywhere, so no pixel is left out.  The
packed form must keep such an L where H = 0.5 and zero L only where H = 0 (the un-windowed marker,
a NaN, on rows h0 / h1 and column 0 of every L plane).  Panoramas 0 and 2 are finite throughout.
"""
import json
import os
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

ZR = PL.ZENITH_RANGE
DEV = "cuda:0"
OUT_W, OUT_H, B = 512, 256, 3
WIDTHS = (128, 256, 512)
BANDS = {128: 47, 256: 93, 512: 185}
INF_PANORAMA, INF_PIXEL = 1, (100, 77)  # (x, y) in tile 0 (256 x 256)
MARKER = 0x7FBADBAD  # the un-windowed marker of a normalised L plane


def _chunks(band, lo, hi):
    """A chunk count whose rows per chunk, ceil(band / n), lie in [lo, hi]."""
    for n in range(1, band + 1):
        r = -(-band // n)
        if lo <= r <= hi and -(-band // r) == n:
            return n
    raise AssertionError(f"no chunking of {band} rows with {lo}..{hi} rows per chunk")


def _case(T, rows=None, T0=None):
    """Depth T on levels 1 and 2 (T0 on level 0, whose band allows depths up to 7); rows =
    (lo, hi): rows per chunk forced into that range on every level that runs depth T."""
    env = {}
    for w in WIDTHS:
        t = T if w != 128 else (T0 if T0 is not None else min(T, 5))
        env[f"PF_JT{w}"] = str(t)
        if t > 2:
            env[f"PF_JTONLY{w}"] = str(t)
        if rows is not None and t == T:  # level 0 at its own depth keeps the planner's chunks
            env[f"PF_JN{w}"] = str(_chunks(BANDS[w], *rows))
    return env


CASES = {
    "T1": _case(1), "T2": _case(2), "T4": _case(4), "T5": _case(5), "T8": _case(8),
    "T10": _case(10),
    "T10-rows1": _case(10, (1, 1)), "T10-rowsLL": _case(10, (3, 3)),
    "T10-drain-g2": _case(10, (6, 11)), "T10-drain-g3": _case(10, (12, 17)),
    "T10-drain-g0": _case(10, (18, 23)), "T10-drain-g1": _case(10, (24, 29)),
    "T8-rows1": _case(8, (1, 1)), "T8-drain-g2": _case(8, (6, 11)),
    "T8-drain-g0": _case(8, (12, 17)),
    "T4-fill-only": _case(4, (5, 5)), "T4-fill-drain": _case(4, (6, 6)),
    "T4-rows1": _case(4, (1, 1)),
    "T5-fill-only": _case(5, (2, 2)), "T5-fill-drain": _case(5, (3, 3)),
    "T1-one-group": _case(1, (2, 2)), "T1-two-groups": _case(1, (3, 3)),
    "T2-fill-only": _case(2, (5, 5)), "T2-fill-drain": _case(2, (6, 6)),
    # 30 jobs per panorama in 8 blocks of 4 waves at levels 1 (3 strips x 10 chunks) and 2
    # (5 strips x 6 chunks): a half-empty last block, three panoramas
    "T10-half-empty-block": dict(_case(10), PF_JN256="10", PF_JN512="6"),
}
GENERAL_CASE = "T10-drain-g2"


@pytest.fixture(scope="module")
def world():
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected on a host without a GPU")
    lay = PL.config_layout("C1")
    seeds = pf_synth.seeds_for(B, 20261021 + 5)
    emap = pf_synth.baseline_emap(seeds, 128, 64).numpy()
    gt = pf_synth.scene_depth(seeds, OUT_W, OUT_H).numpy()
    tiles, total = O.make_tiles(lay)
    resp = pf_synth.responses(seeds, lay.ntiles)
    nt = lay.ntiles
    data = np.stack([O.warp_depth(gt[b], tiles, total, O.responses(resp[b * nt:(b + 1) * nt]))
                     for b in range(B)])
    data[INF_PANORAMA, tiles[0].offset + INF_PIXEL[1] * 256 + INF_PIXEL[0]] = np.inf
    levels, u16, infs = [], [], []
    for b in range(B):
        prev, planes = None, []
        for level in range(3):
            lv = O.level_dims(OUT_W, OUT_H, ZR, level)
            assert (lv.w, lv.h1 - lv.h0 + 1) == (WIDTHS[level], BANDS[WIDTHS[level]])
            seed = O.seed_level0(emap[b], lv) if level == 0 else O.upsample(prev, lv)
            rL, rn, oops, _ = O.targets(tiles, data[b], lv)
            assert oops == 0
            ln = O.normalize(rL, rn, lv)
            marker = ln.view(np.uint32) == MARKER
            assert marker[lv.h0:lv.h1 + 1].any()
            assert not (np.isnan(ln) & ~marker).any(), "the oracle's targets hold a NaN"
            if b == INF_PANORAMA:
                infs.append((int(np.isposinf(ln).sum()), int(np.isneginf(ln).sum())))
            else:
                assert np.isfinite(ln[~marker]).all()
            prev = O.jacobi(seed, ln, lv, lv.iters)
            planes.append(prev)
        out, oops = O.solve_depth_all(emap[b], tiles, data[b], OUT_W, ZR)
        assert oops == 0 and all(np.isfinite(a).all() for a in planes)
        levels.append(planes)
        u16.append(out)
    assert infs[0] == (1, 4) and infs[2] == (1, 4), infs  # covered pixels with L = +inf / -inf
    for p in levels:
        for a in p:
            a.setflags(write=False)
    return {"lay": lay, "emap": emap, "data": data, "levels": levels, "u16": np.stack(u16)}


def _gpu(emap, data, env):
    """The level planes [B][3] and the u16 panoramas [B, h, w] under the forced plan."""
    lay = PL.config_layout("C1")
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    f = panofuse.Fuser(0)
    try:
        f.set_tiles(lay)
        f.set_jacobi_engine(resident=False)
        t_emap = torch.from_numpy(np.ascontiguousarray(emap)).to(DEV)
        t_data = torch.from_numpy(np.ascontiguousarray(data)).to(DEV).reshape(B, -1).contiguous()
        planes = []
        for b in range(B):
            prev, mine = None, []
            for level in range(3):
                lv = O.level_dims(OUT_W, OUT_H, ZR, level)
                lsum = torch.zeros(lv.h * lv.w, dtype=torch.float32, device=DEV)
                cnt = torch.zeros_like(lsum)
                f.fuse_partial(t_data[b], None, 0, lay.ntiles, OUT_W, ZR, level, lsum, cnt)
                buf = torch.zeros(lv.h * lv.w, dtype=torch.float32, device=DEV)
                f.fuse_level(t_emap[b:b + 1] if level == 0 else None, prev, lsum, cnt, OUT_W, ZR,
                             level, buf)
                prev = buf
                mine.append(buf)
            torch.cuda.synchronize()
            planes.append([m.cpu().numpy() for m in mine])
        out = torch.zeros((B, OUT_H, OUT_W), dtype=torch.int16, device=DEV)
        f.fuse(t_emap, t_data, out, ZR)
        torch.cuda.synchronize()
        return planes, out.cpu().numpy().view(np.uint16)
    finally:
        f.close()
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _mismatches(levels, u16_ref, planes, u16):
    """Differing values per panorama and level, and differing u16 pixels."""
    bad = [[int((planes[b][lv].reshape(levels[b][lv].shape).view(np.uint32)
                 != levels[b][lv].view(np.uint32)).sum()) for lv in range(3)] for b in range(B)]
    return {"levels": bad, "u16": int((u16 != u16_ref).sum()), "nonzero": int(np.count_nonzero(u16))}


def _child(inputs_path, out_path, names):
    """Runs in a fresh process: every named case against the oracle's planes of inputs_path; a
    `case NAME` line on stderr ahead of each case's PF_JPLAN lines."""
    z = np.load(inputs_path)
    levels = [[z[f"p{b}{lv}"] for lv in range(3)] for b in range(B)]
    res = {}
    for name in names.split(","):
        print(f"case {name}", file=sys.stderr, flush=True)
        planes, u16 = _gpu(z["emap"], z["data"], CASES[name])  # an error ends the process here
        res[name] = _mismatches(levels, z["u16"], planes, u16)
        with open(out_path, "w") as fh:  # after every case: what ran before an error is kept
            json.dump(res, fh)


CHILD = ("import sys; sys.path[:0] = [{pkg!r}, {oracle!r}, {tests!r}]; "
         "import test_gpu_jacobi_lead as t; t._child(sys.argv[1], sys.argv[2], sys.argv[3])")


def _run_child(world, tmp, names, extra_env):
    """The planner's engine switches (PF_JPIPE, PF_JSLOW) and PF_JPLAN are read once per process,
    so the cases run in one fresh child process, which ends at the first case that raises (a GPU
    error among them): nothing more starts on the GPU, the cases before it keep their own verdict
    and the ones after it fail as not run.  Returns {case: mismatches}, {case: plan lines}, the
    child's exit status and the end of its stderr."""
    inputs_path, out_path = tmp / "inputs.npz", tmp / "result.json"
    np.savez(inputs_path, emap=world["emap"], data=world["data"], u16=world["u16"],
             **{f"p{b}{lv}": world["levels"][b][lv] for b in range(B) for lv in range(3)})
    env = dict(os.environ, PF_JPLAN="1", **extra_env)
    code = CHILD.format(pkg=os.path.dirname(os.path.abspath(panofuse.__file__)),
                        oracle=os.path.dirname(os.path.abspath(O.__file__)),
                        tests=os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code, str(inputs_path), str(out_path),
                        ",".join(names)], env=env, capture_output=True, text=True, timeout=300)
    plans, cur = {}, None
    for ln in r.stderr.splitlines():
        if ln.startswith("case "):
            cur = plans.setdefault(ln[5:], [])
        elif ln.startswith("jacobi plan") and cur is not None:
            cur.append(ln)
    res = {}
    if out_path.exists():
        with open(out_path) as fh:
            res = json.load(fh)
    return res, plans, r.returncode, r.stderr[-2000:]


def _check(run, name, form):
    res, plans, rc, err = run
    if name not in res:
        ran = list(plans)
        if ran and ran[-1] == name:
            pytest.fail(f"{name}: the child process ended with status {rc} in this case:\n{err}")
        pytest.fail(f"{name}: not run, the child process ended with status {rc} in case "
                    f"{ran[-1] if ran else None}")
    # the plan lines: the form, the single-wave engine (no `p` mark), the forced depth and chunks
    env = CASES[name]
    assert plans[name] and all(f" {form} C2:" in ln for ln in plans[name]), plans[name]
    for w in WIDTHS:
        mine = [ln for ln in plans[name] if ln.startswith(f"jacobi plan {w}x")]
        assert len(mine) == B + 1, mine  # one per panorama (pf_fuse_level) and the batched fusion
        for ln in mine:
            passes = ln.split(":", 1)[1].split()
            assert not any(p.endswith("p") for p in passes), ln
            want = f"T{env[f'PF_JT{w}']}/"
            if f"PF_JN{w}" in env:
                want += f"n{env[f'PF_JN{w}']}"
            assert any(p.startswith(want) for p in passes), (want, ln)
    got = res[name]
    for b in range(B):
        for lv in range(3):
            assert got["levels"][b][lv] == 0, (
                f"{name}: panorama {b} level {lv}: {got['levels'][b][lv]} Jacobi values differ")
    assert got["u16"] == 0, f"{name}: {got['u16']} u16 pixels differ from the oracle's fusion"
    assert got["nonzero"] > 0


@pytest.fixture(scope="module")
def packed(world, tmp_path_factory):
    return _run_child(world, tmp_path_factory.mktemp("packed"), list(CASES), {"PF_JPIPE": "0"})


@pytest.mark.parametrize("name", list(CASES))
def test_forced_depth_and_chunks_match_oracle(packed, name):
    _check(packed, name, "packed")


def test_general_form_matches_oracle(world, tmp_path):
    """The general (scalar) form takes the same loads: one depth and chunking under PF_JSLOW."""
    run = _run_child(world, tmp_path, [GENERAL_CASE], {"PF_JSLOW": "1", "PF_JPIPE": "0"})
    _check(run, GENERAL_CASE, "general")
