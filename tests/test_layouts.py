"""The reference's four tile tables (leres, midas, fold4, fold3), layout files, and what the CPU
oracle says about them -- CPU only.

tests/golden/layout_tables.json holds the integer degrees of the four tables of the reference's
main() (Main.cpp:695-887) and the RGB export's tile heights: settings only.  The Python tables
(pf_layouts.py) and the C++ ones (csrc/pf_layouts.cpp through pfd_layout) must agree with it to
1e-4 degrees and with each other bit for bit; the tile names, the 359.9 degree cap and the layout
file rules are checked on both sides.  The oracle facts pin the out-of-tile tap counts that make
these layouts new test ground for the GPU kernels (tests/test_gpu_layouts.py)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import panofuse
import pf_layouts as PL
import pyoracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(os.path.dirname(panofuse.LIB_PATH))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "layout_tables.json")))["tables"]
ZR = PL.ZENITH_RANGE

PY = {"leres": PL.leres_layout, "midas": PL.midas_layout, "fold4": PL.fold4_layout,
      "fold3": PL.fold3_layout}
CFG = {"leres": "LERES", "midas": "MIDAS", "fold4": "FOLD4", "fold3": "FOLD3"}
NTILES = {"leres": 15, "midas": 15, "fold4": 12, "fold3": 9}
FIRST_LAST = {"leres": ("-3_75_18_94", "285_363_86_162"),
              "midas": ("-2_74_20_78", "286_362_102_160"),
              "fold4": ("-2_92_17_109", "268_362_71_163"),
              "fold3": ("-2_122_12_120", "238_362_60_168")}


@pytest.fixture(scope="module")
def dlib():
    L = C.CDLL(os.path.join(PKG, "lib", "libpanofuse_depth.so"))
    L.pfd_layout.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_int]
    L.pfd_layout.restype = C.c_int
    L.pfd_rgb_tile_size.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.pfd_rgb_tile_size.restype = None
    L.pfd_leres_layout.argtypes = [C.c_void_p, C.c_void_p]
    L.pfd_leres_layout.restype = None
    return L


def _c_layout(dlib, spec, cap=PL.MAX_TILES):
    f = np.zeros((cap, 4), np.float32)
    r = np.zeros((cap, 4), np.float32)
    n = dlib.pfd_layout(os.fsencode(spec), f.ctypes.data, r.ctypes.data, cap)
    return n, f[:max(n, 0)], r[:max(n, 0)]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _degrees(a):
    return np.asarray(a, np.float64) / PL.MYPI * 180.0


@pytest.mark.parametrize("name", sorted(PY))
def test_tables_match_the_golden_degrees_and_each_other(dlib, name):
    lay = PY[name]()
    gold = GOLDEN[name]
    assert lay.ntiles == NTILES[name] == len(gold["fov"]) == len(gold["range"])
    assert np.abs(_degrees(lay.fovs) - np.array(gold["fov"])).max() < 1e-4
    assert np.abs(_degrees(lay.ranges) - np.array(gold["range"])).max() < 1e-4
    n, f, r = _c_layout(dlib, name)
    assert n == lay.ntiles
    assert np.array_equal(_bits(f), _bits(lay.fovs))
    assert np.array_equal(_bits(r), _bits(lay.ranges))
    cfg = PL.config_layout(CFG[name])
    assert np.array_equal(_bits(cfg.fovs), _bits(lay.fovs))
    assert np.array_equal(_bits(cfg.ranges), _bits(lay.ranges))
    # the count alone, and a capacity that is too small
    assert dlib.pfd_layout(name.encode(), None, None, 0) == lay.ntiles
    assert _c_layout(dlib, name, cap=lay.ntiles - 1)[0] == -1


def test_unknown_names(dlib, capfd):
    assert dlib.pfd_layout(b"nosuch", None, None, 0) == -1
    assert dlib.pfd_layout(None, None, None, 0) == -1
    with pytest.raises(ValueError):
        PL.config_layout("NOSUCH")


def test_leres_is_unchanged(dlib):
    """pfd_leres_layout and pfd_layout("leres") are one table, the default of every command."""
    f = np.zeros((15, 4), np.float32)
    r = np.zeros((15, 4), np.float32)
    dlib.pfd_leres_layout(f.ctypes.data, r.ctypes.data)
    n, f2, r2 = _c_layout(dlib, "leres")
    assert n == 15 and np.array_equal(_bits(f), _bits(f2)) and np.array_equal(_bits(r), _bits(r2))
    lay = PL.config_layout("LERES")
    assert (int(lay.tile_w[0]), int(lay.tile_h[0])) == (1024, 988)


@pytest.mark.parametrize("name", sorted(PY))
def test_tile_names_and_export_sizes(dlib, name):
    lay = PY[name]()
    names = PL.tile_names(lay)
    assert (names[0], names[-1]) == FIRST_LAST[name]
    # every name is the golden table's integer degrees
    assert names == ["_".join(str(v) for v in f) for f in GOLDEN[name]["fov"]]
    want = tuple(GOLDEN[name]["export_tile"])
    assert (int(lay.tile_w[0]), int(lay.tile_h[0])) == want  # the default size of the table
    for f in lay.fovs:
        w, h = C.c_int(0), C.c_int(0)
        dlib.pfd_rgb_tile_size(np.ascontiguousarray(f).ctypes.data, C.byref(w), C.byref(h))
        assert (w.value, h.value) == want
        assert PL.rgb_tile_size(f) == want


@pytest.mark.parametrize("name", sorted(PY))
def test_range_cap_on_the_last_sector(name):
    """MergeDepthMaps stores MIN2(range, D2R(359.9)): the last sector's 360 degree edge."""
    lay = PY[name]()
    capped = lay.capped_ranges()
    nsec = lay.ntiles // 3
    cap = np.float32(PL.RANGE_CAP)
    for band in range(3):
        last = band * nsec + nsec - 1
        assert float(lay.ranges[last, 0]) >= PL.RANGE_CAP  # 360 degrees before the cap
        assert capped[last, 0] == cap
        assert np.array_equal(_bits(capped[last, 1:]), _bits(lay.ranges[last, 1:]))
    others = [i for i in range(lay.ntiles) if i % nsec != nsec - 1]
    assert np.array_equal(_bits(capped[others]), _bits(lay.ranges[others]))
    # the oracle's tiles carry the capped ranges
    tiles, _ = O.make_tiles(lay)
    assert np.float32(tiles[lay.ntiles - 1].ranges[0]) == cap


def _file_text(name, header="# az_left az_right zen_top zen_down  range: the same four\n"):
    g = GOLDEN[name]
    rows = ["%d %d %d %d\t%d %d %d %d" % (*f, *r) for f, r in zip(g["fov"], g["range"])]
    return header + "\n".join(rows[:3]) + "\n\n   # a comment line\n" + "\r\n".join(rows[3:])


def test_fold4_file_is_fold4_bit_for_bit(dlib, tmp_path):
    p = tmp_path / "fold4.txt"
    p.write_text(_file_text("fold4"))
    want = PL.fold4_layout(256, 200)
    lay = PL.load_layout_file(str(p), 256, 200)
    assert lay.ntiles == 12 and int(lay.tile_w[3]) == 256 and int(lay.tile_h[3]) == 200
    assert np.array_equal(_bits(lay.fovs), _bits(want.fovs))
    assert np.array_equal(_bits(lay.ranges), _bits(want.ranges))
    n, f, r = _c_layout(dlib, str(p))
    assert n == 12
    assert np.array_equal(_bits(f), _bits(want.fovs)) and np.array_equal(_bits(r), _bits(want.ranges))
    # decimal forms of the same degrees
    q = tmp_path / "fold4_dec.txt"
    q.write_text(_file_text("fold4").replace("92", "9.2e1").replace("-2", "-2.000"))
    n, f, r = _c_layout(dlib, str(q))
    assert n == 12 and np.array_equal(_bits(f), _bits(want.fovs))
    assert np.array_equal(_bits(PL.load_layout_file(str(q), 8, 8).fovs), _bits(want.fovs))


def test_leres_file_is_close_but_not_leres(dlib, tmp_path):
    """leres' edges come from float additions: the file's single rounding of D2R(deg) gives the
    same windows to 1e-4 degrees, not the same bits."""
    p = tmp_path / "leres.txt"
    p.write_text(_file_text("leres"))
    want = PL.leres_layout()
    lay = PL.load_layout_file(str(p), 1024, 988)
    n, f, r = _c_layout(dlib, str(p))
    assert n == 15 and np.array_equal(_bits(f), _bits(lay.fovs))
    assert np.array_equal(_bits(r), _bits(lay.ranges))
    assert np.abs(_degrees(lay.fovs) - _degrees(want.fovs)).max() < 1e-4
    assert np.abs(_degrees(lay.ranges) - _degrees(want.ranges)).max() < 1e-4
    # the windows happen to round alike; twelve range edges (azi - margin in float) do not
    assert int((_bits(lay.ranges) != _bits(want.ranges)).sum()) == 12


GOOD = "0 90 45 135 90 0 60 120\n"
MALFORMED = {
    "seven": "0 90 45 135 90 0 60\n",
    "nine": GOOD + "0 90 45 135 90 0 60 120 7\n",
    "word": "0 90 45 135 90 0 sixty 120\n",
    "nan": "0 90 45 135 90 0 nan 120\n",
    "inf": "0 90 45 135 90 0 inf 120\n",
    "overflow": "0 90 45 135 90 0 1e999 120\n",
    "float_overflow": "0 90 45 135 90 0 1e200 120\n",
    "hex": "0 90 45 135 90 0 0x3c 120\n",
    "comma": "0,90,45,135,90,0,60,120\n",
    "empty": "",
    "comments_only": "# nothing\n\n   \n# here\n",
    "too_many": GOOD * (PL.MAX_TILES + 1),
}


@pytest.mark.parametrize("case", sorted(MALFORMED))
def test_malformed_files_are_rejected(dlib, tmp_path, case):
    p = tmp_path / (case + ".txt")
    p.write_text(MALFORMED[case])
    assert _c_layout(dlib, str(p))[0] == -1
    with pytest.raises(ValueError):
        PL.load_layout_file(str(p), 64, 64)


def test_limits_of_a_good_file(dlib, tmp_path):
    p = tmp_path / "max.txt"
    p.write_text(GOOD * PL.MAX_TILES)  # exactly the limit
    assert _c_layout(dlib, str(p))[0] == PL.MAX_TILES
    assert PL.load_layout_file(str(p), 64, 64).ntiles == PL.MAX_TILES
    q = tmp_path / "noeol.txt"
    q.write_text("  +0. 9e1 .45e2 135.0 90 -0 60 120 # no newline at the end")
    n, f, r = _c_layout(dlib, str(q))
    lay = PL.load_layout_file(str(q), 64, 64)
    assert n == 1 and np.array_equal(_bits(f), _bits(lay.fovs))
    assert np.array_equal(_bits(r), _bits(lay.ranges))
    assert lay.fovs[0, 1] == np.float32(PL.D2R(90)) and lay.fovs[0, 2] == np.float32(PL.D2R(45))
    assert _c_layout(dlib, str(tmp_path / "missing.txt"))[0] == -1
    with pytest.raises(OSError):
        PL.load_layout_file(str(tmp_path / "missing.txt"), 64, 64)


# taps_outside per level (pfo_targets' oops) at output widths 512 and 2048: geometry only.
TAPS_OUTSIDE = {"leres": {512: (58, 0, 0), 2048: (0, 0, 0)},
                "midas": {512: (217, 35, 0), 2048: (0, 0, 0)},
                "fold4": {512: (103, 48, 0), 2048: (0, 0, 0)},
                "fold3": {512: (46, 0, 0), 2048: (0, 0, 0)}}
# taps_clamped per level (oob) at 512 with 256 x 256 tiles (leres: 256 x 247)
TAPS_CLAMPED_512 = {"leres": (8, 0, 0), "midas": (133, 30, 0), "fold4": (3, 0, 0),
                    "fold3": (1, 0, 0)}
UNCOVERED = {"leres": {512: (0, 0, 0), 2048: (0, 0, 729)},
             "midas": {512: (0, 0, 0), 2048: (0, 0, 729)},
             "fold4": {512: (0, 0, 0), 2048: (0, 0, 729)},
             "fold3": {512: (0, 0, 511), 2048: (511, 1023, 2775)}}


@pytest.mark.parametrize("name", sorted(PY))
def test_oracle_facts(name):
    lay = PY[name](256, 247 if name == "leres" else 256)
    tiles, total = O.make_tiles(lay)
    data = np.zeros(total, np.float32)
    for out_w in (512, 2048):
        for level in range(3):
            lv = O.level_dims(out_w, out_w // 2, ZR, level)
            _, n, oops, oob = O.targets(tiles, data, lv)
            assert oops == TAPS_OUTSIDE[name][out_w][level], (out_w, level)
            assert oob == (TAPS_CLAMPED_512[name][level] if out_w == 512 else 0), (out_w, level)
            assert n.max() <= 2
            assert int((n[lv.h0 + 1:lv.h1, 1:] == 0).sum()) == UNCOVERED[name][out_w][level]
