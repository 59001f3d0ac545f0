"""The facade's ErrorCompare entry points through a compiled caller -- CPU only.

tests/cpp/compare_link.cpp includes include/pf_depth.h and is linked against
libpanofuse_depth.so (bin/pf_compare_link, built by the package Makefile like pf_facade_check).
* DepthNamespace::ErrorCompare with the reference's signature (Depth.h:318-319) on a missing gt
  file returns false after the reference's "cannot load emap_gt? ..." line; the loads come before
  any GPU call, so this runs on a host without a GPU.
* EquirectangularMap::Save8bit (Depth.cpp:612-635) of a 5x3 map with values below 0 and above 1
  writes the bytes that the reference's stbi_write_png wrote for the same plane
  (tests/golden/compare_ref.npz: save8_plane, save8_png).
* Save8BitPNG, the writer behind both, reproduces the reference's PNG file byte for byte for
  every shifted plane of the golden (written there by stbi_write_png as the reference's program
  builds it).
* The libraries export the new entry points."""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np

import compare_ref as R
import panofuse

PKG = os.path.dirname(os.path.dirname(panofuse.LIB_PATH))
BIN = os.path.join(PKG, "bin", "pf_compare_link")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "compare_ref.npz")


def test_missing_file_and_save8bit(tmp_path):
    assert os.path.exists(BIN), f"{BIN} not built (make -C {PKG})"
    r = subprocess.run([BIN, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert "RET 0" in lines and "SAVE 1" in lines, r.stdout
    assert f"cannot load emap_gt? {tmp_path}/no_such_gt.png" in lines
    assert lines.index(f"cannot load emap_gt? {tmp_path}/no_such_gt.png") < lines.index("RET 0")
    assert "cannot load emap_baseline?" not in r.stdout  # the gt comes first and ends the call
    assert not (tmp_path / "shifted.png").exists()
    z = np.load(GOLDEN)
    i = np.arange(15, dtype=np.float32)
    v = ((i * np.float32(0.1)).astype(np.float32) - np.float32(0.25)).reshape(3, 5)
    assert v.min() < 0 and v.max() > 1
    assert np.array_equal(R.save8bit(v), z["save8_plane"])
    assert (tmp_path / "save8.png").read_bytes() == z["save8_png"].tobytes()


def test_png_writer_reproduces_every_golden_file(tmp_path):
    """The facade's one-channel 8-bit writer on the reference's shifted planes (host code: called
    through its C++ symbol)."""
    path = os.path.join(PKG, "lib", "libpanofuse_depth.so")
    syms = subprocess.run(["nm", "-D", path], capture_output=True, text=True, check=True).stdout
    name = [ln.split()[-1] for ln in syms.splitlines() if "Save8BitPNG" in ln]
    assert len(name) == 1, syms
    fn = getattr(C.CDLL(path), name[0])
    fn.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_char_p]
    fn.restype = C.c_bool
    z = np.load(GOLDEN)
    planes = sorted(k for k in z.files if k.startswith("pixels"))
    assert len(planes) >= 15
    filters = set()
    for k in planes:
        px = np.ascontiguousarray(z[k])
        out = tmp_path / (k + ".png")
        assert fn(px.tobytes(), px.shape[1], px.shape[0], str(out).encode())
        want = z["png" + k[len("pixels"):]].tobytes()
        assert out.read_bytes() == want, k
        raw = zlib.decompress(want[41:41 + int.from_bytes(want[33:37], "big")])
        filters |= {raw[y * (px.shape[1] + 1)] for y in range(px.shape[0])}
    assert len(filters) >= 3, filters  # the row-filter choice is exercised, not one constant type


def test_exports():
    lib = C.CDLL(panofuse.LIB_PATH)
    for name in ("pf_error_compare", "pf_disp_depth_convert"):
        assert hasattr(lib, name) and name in panofuse.EXPORTS
    out = subprocess.run(["nm", "-DC", os.path.join(PKG, "lib", "libpanofuse_depth.so")],
                         capture_output=True, text=True, check=True).stdout
    s = "std::__cxx11::basic_string<char, std::char_traits<char>, std::allocator<char> >"
    want = (f"DepthNamespace::ErrorCompare({s}&, {s}&, bool, float&, float&, float&, float&, "
            "float&, float&, float&, int, bool, char const*)",
            "DepthNamespace::EquirectangularMap::DispDepthConversion()",
            f"DepthNamespace::EquirectangularMap::Save8bit({s}&)")
    for w in want:
        assert any(line.endswith(" T " + w) for line in out.splitlines()), w
