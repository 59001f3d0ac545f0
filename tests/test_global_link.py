"""The facade's post-fusion calibration entry points through a compiled caller -- CPU only.

tests/cpp/global_link.cpp includes include/pf_depth.h and is linked against
libpanofuse_depth.so (bin/pf_global_link, built by the package Makefile like pf_compare_link).
* DepthNamespace::MedianScaling (Depth.h:337) on a map without any valid pixel returns false
  after the reference's "MedianScaling: zero val0_median ??" line, with the map and the median
  outputs untouched; the check comes before any GPU call, so this runs on a host without a GPU.
* The libraries export the reference's manglings and the four C-ABI names."""
import ctypes as C
import os
import subprocess

import panofuse

PKG = os.path.dirname(os.path.dirname(panofuse.LIB_PATH))
BIN = os.path.join(PKG, "bin", "pf_global_link")


def test_median_scaling_without_valid_pixels():
    assert os.path.exists(BIN), f"{BIN} not built (make -C {PKG})"
    env = dict(os.environ, HIP_VISIBLE_DEVICES="")  # no device is needed, so none is offered
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines == ["MedianScaling: zero val0_median ??", "RET 0", "UNTOUCHED 1",
                     "MedianScaling: zero val0_median ??", "RET 0"], r.stdout
    assert "[panofuse]" not in r.stdout  # no context was made


def test_exports():
    lib = C.CDLL(panofuse.LIB_PATH)
    for name in ("pf_register_global", "pf_result_transform", "pf_median_scale",
                 "pf_copy_invalid"):
        assert hasattr(lib, name) and name in panofuse.EXPORTS
    out = subprocess.run(["nm", "-DC", os.path.join(PKG, "lib", "libpanofuse_depth.so")],
                         capture_output=True, text=True, check=True).stdout
    emap = "DepthNamespace::EquirectangularMap"
    want = (f"DepthNamespace::SolveDepthToDepth2({emap}&, unsigned short*, int, int, "
            "Imath::Vec2<float>&, Imath::Vec4<float>&)",
            f"DepthNamespace::MedianScaling({emap}&, {emap}&, float*, float*)",
            f"{emap}::CopyInvalidPixels({emap}&)",
            "DepthNamespace::TransformResult(unsigned short*, int, int, Imath::Vec2<float>&, "
            "Imath::Vec4<float>&)")
    for w in want:
        assert any(line.endswith(" T " + w) for line in out.splitlines()), w
