"""Off-grid, mixed and multi-channel tile shapes on the CPU: the cases of tests/tile_shapes.py
checked against the host probe and the oracle, before tests/test_gpu_tile_shapes.py runs them on
the GPU.

* The numpy restatement of the depth warp's patch classification reproduces the table in
  tests/test_gpu_parity.py::test_warp_depth_ragged_batch_and_resize for plain C1, and on the
  mixed layout every one of the eight staging paths gets a patch cut in X and one cut in Y over
  the five panorama sizes -- a condition the case list must satisfy, not a measurement.
* The float32 numpy gather equals the oracle's depth warp bit for bit on the mixed layout, so the
  GPU test has two checkers that share no code.
* The oracle with channels = 3: the warp writes channel 0 only, the merge, the tap maps, the
  smoothing solver and the registration samples equal the 1-channel run, and the other channels
  keep what they held.  MiDaS 40 x 30 has clamped taps at level 0, so the clamp to
  n - channels is part of what is compared.
* The staged RGB warp's host tables for the RGB case tiles, replayed on the host.
"""
import os
import subprocess

import numpy as np
import pytest

import panofuse
import pf_layouts as PL
import pf_synth
import pyoracle as O
import tile_shapes as TS

ZR = PL.ZENITH_RANGE


def test_classification_reproduces_the_c1_table():
    lay = PL.config_layout("C1")
    for pano, want in TS.C1_TABLE.items():
        got = TS.classify(lay, *pano)
        assert TS.path_counts(got) == want, pano
        assert set(k for _, k in got) == {"full"}  # 256 x 256: whole patches only


@pytest.fixture(scope="module")
def mixed_table():
    return TS.classification_table(TS.MIXED_SIZES)


def test_mixed_layout_cuts_a_patch_in_x_and_y_on_every_path(mixed_table):
    print("\n" + TS.format_table(mixed_table))
    cond = TS.cut_condition(mixed_table)
    assert cond == {path: (True, True) for path in TS.PATHS}, cond
    for (pw, ph), c in mixed_table.items():
        # every patch is classified: ceil(w/64) * ceil(h/32) per tile
        assert sum(c.values()) == sum(-(-w // 64) * -(-h // 32) for w, h in TS.MIXED_SIZES)
        assert all(path.startswith("rag" if pw % 4 == 0 else "box") for path, _ in c)


def test_small_layout_patches_are_all_cut():
    """The smallest tiles: one patch each but 65 x 2 (two) and 2 x 33 (two), every one cut."""
    for pano in ((512, 256), (302, 151)):
        c = TS.classify(TS.layout_with(TS.SMALL_SIZES), *pano)
        assert sum(c.values()) == 8
        assert not any(k == "full" for _, k in c)


@pytest.mark.parametrize("pw,ph", [(512, 256), (302, 151)])
def test_numpy_gather_equals_the_oracle_warp(pw, ph):
    lay = TS.layout_with(TS.MIXED_SIZES)
    tiles, total = O.make_tiles(lay)
    assert total == TS.tile_elems(lay)
    gt = pf_synth.scene_depth(pf_synth.seeds_for(1, 4242), pw, ph)[0].numpy()
    ref = O.warp_depth(gt, tiles, total, None)
    got = TS.warp_depth_gather(gt, lay)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert np.unique(ref).size > total // 2  # a scene, not a constant


@pytest.mark.parametrize("cfg", ["MIDAS", "LERES"])
def test_oracle_three_channels_equal_one(cfg):
    k = TS.channel_case(cfg)
    t1, n1, t3, n3 = k["t1"], k["n1"], k["t3"], k["n3"]
    emap, gt, d1, d3 = k["emaps"][0], k["gts"][0], k["d1"][0], k["d3"][0]
    for a, b in zip(t1, t3):
        assert b.offset == 3 * a.offset and b.channels == 3

    # the warp writes channel 0 only
    w3 = TS.oracle_warp_filled(gt, t3, n3)
    assert np.array_equal(TS.channel(w3, 0), O.warp_depth(gt, t1, n1))
    assert TS.fill_kept(w3)

    # the merge: same coefficients and u16; the transform touches channel 0 only
    x1, x3 = d1.copy(), d3.copy()
    r1, a1 = O.merge(emap, t1, x1, TS.OUT_W, ZR)
    r3, a3 = O.merge(emap, t3, x3, TS.OUT_W, ZR)
    assert np.array_equal(a1, a3) and np.array_equal(r1, r3)
    assert np.array_equal(TS.channel(x3, 0), x1) and TS.fill_kept(x3)
    assert int((r1 != 0).sum()) > TS.OUT_W

    # the tap maps: 3 x the 1-channel indices, clamped taps included
    clamped = 0
    for level in range(O.num_levels(TS.OUT_W)):
        lv = O.level_dims(TS.OUT_W, TS.OUT_W // 2, ZR, level)
        p1, p3 = O.probe_taps(t1, lv), O.probe_taps(t3, lv)
        assert np.array_equal(np.where(p1 >= 0, p1 * 3, -1), p3), level
        _, _, _, oob = O.targets(t3, d3, lv)
        assert oob == O.targets(t1, d1, lv)[3]
        clamped += oob
    assert clamped > 0  # the clamp to n - channels is exercised
    if cfg == "MIDAS":
        lv = O.level_dims(TS.OUT_W, TS.OUT_W // 2, ZR, 0)
        assert O.targets(t3, d3, lv)[2:] == (217, 44)

    # the smoothing solver
    s1 = O.solve_smoothing(t1, d1, 256, 128, ZR)
    s3 = O.solve_smoothing(t3, d3, 256, 128, ZR)
    assert np.array_equal(s1, s3) and int((s1 != 0).sum()) > 256

    # the registration samples
    for a, b in zip(t1, t3):
        xs1, ys1, c1, rows1 = O.reg_samples(a, d1, emap, ZR)
        xs3, ys3, c3, rows3 = O.reg_samples(b, d3, emap, ZR)
        assert (c1, rows1) == (c3, rows3)
        assert np.array_equal(xs1, xs3) and np.array_equal(ys1, ys3)
        assert not (xs3 == float(TS.FILL)).any()


def test_interleave_helpers():
    d = np.arange(12, dtype=np.float32).reshape(2, 6)
    d3 = TS.interleave(d)
    assert d3.shape == (2, 18) and np.array_equal(TS.channel(d3, 0), d)
    assert (TS.channel(d3, 1) == TS.FILL).all() and (TS.channel(d3, 2) == TS.FILL).all()
    lay = TS.layout_with(TS.MIXED_SIZES)
    sl = TS.tile_slices(lay, 3)
    assert sl[0] == slice(0, 100 * 70 * 3) and sl[-1].stop == TS.tile_elems(lay, 3)


RGB_TABLES = os.path.join(os.path.dirname(os.path.dirname(panofuse.LIB_PATH)), "bin",
                          "pf_rgb_tables")


@pytest.mark.parametrize("pw,ph", [(512, 256), (1024, 512), (48, 24)])
def test_rgb_warp_host_tables_replay(pw, ph):
    """The staged RGB warp's host tables for the RGB case tiles, replayed on the host by
    tests/cpp/rgb_tables_check.cpp: every staged pixel's LDS locations hold the texels of its
    taps and every unit lies inside the panorama.  These tiles' rows are more than two panorama
    rows apart, so a patch's footprint has rows no corner reads: rgb_footprint once ran its unit
    arithmetic on their INT32_MAX / INT32_MIN bounds and rgb_patches_host wrote outside its unit
    table (the GPU run of tests/test_gpu_tile_shapes.py::test_warp_rgb_partial_columns crashed in
    the host code).  At 48 x 24 single tile rows are wider than half the panorama: those patches
    must be marked wide, not staged with an empty footprint."""
    assert os.path.exists(RGB_TABLES), f"{RGB_TABLES} not built (make -C the package)"
    lay = TS.layout_with(TS.RGB_SIZES)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="")  # host code only
    staged = wide = 0
    for p in range(lay.ntiles):
        args = [RGB_TABLES, str(lay.tile_w[p]), str(lay.tile_h[p]), str(pw), str(ph)]
        args += [repr(float(v)) for v in lay.fovs[p]]
        r = subprocess.run(args, capture_output=True, text=True, timeout=60, env=env)
        print(r.stdout.strip())
        assert r.returncode == 0, (p, r.returncode, r.stdout + r.stderr[-2000:])
        words = r.stdout.split()
        assert words[-1] == "0" and words[-2] == "bad"
        staged += int(words[words.index("staged_pixels") + 1])
        wide += int(words[words.index("wide") + 1])
    assert staged > 0
    if (pw, ph) == (48, 24):
        assert wide > 0
