"""GPU end-to-end of the disparity-tile path above the C-ABI: the mode-0 command line with
--tile-model disparity, and the facade's SolveDisparityToDepth / D2DTransform /
MergeDisparityMaps called from compiled C++ (tests/cpp/disp_check.cpp).  Both are held to the
binding (panofuse.Fuser.merge_disparity / register_disparity), which tests/test_gpu_disp.py holds
to the CPU restatement bit for bit."""
import math
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import panofuse  # noqa: E402
import pf_layouts as PL  # noqa: E402
import pf_synth  # noqa: E402
import pyoracle as O  # noqa: E402

PKG = os.path.dirname(os.path.dirname(panofuse.LIB_PATH))
MAIN = os.path.join(PKG, "bin", "panofuse_main")
CHECK = os.path.join(PKG, "bin", "pf_disp_check")
DEPTH_LIB = os.path.join(PKG, "lib", "libpanofuse_depth.so")
MYPI = 3.14159265359
ZR = PL.ZENITH_RANGE
DEV = "cuda:0"


def _png16_write(path, a):
    h, w = a.shape
    raw = b"".join(b"\0" + a[y].astype(">u2").tobytes() for y in range(h))

    def chunk(t, d):
        return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d))
    open(path, "wb").write(b"\x89PNG\r\n\x1a\n" +
                           chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 16, 0, 0, 0, 0)) +
                           chunk(b"IDAT", zlib.compress(raw, 1)) + chunk(b"IEND", b""))


def _png16_read(path):
    d = open(path, "rb").read()
    pos, idat = 8, b""
    while pos < len(d):
        n = struct.unpack(">I", d[pos:pos + 4])[0]
        t, body = d[pos + 4:pos + 8], d[pos + 8:pos + 8 + n]
        if t == b"IHDR":
            w, h = struct.unpack(">II", body[:8])
        elif t == b"IDAT":
            idat += body
        pos += 12 + n
    raw = zlib.decompress(idat)
    return np.frombuffer(b"".join(raw[y * (2 * w + 1) + 1:(y + 1) * (2 * w + 1)]
                                  for y in range(h)), ">u2").reshape(h, w).astype(np.uint16)


def _cround(x):  # C round(): half away from zero
    return int(math.copysign(math.floor(abs(x) + 0.5), x))


def _q16(a):
    return (np.clip(a, 0, 1) * 65535.0 + 0.5).astype(np.uint16)


def _disparity(depth, tiles):
    """Per-tile normalised inverse depth (MiDaS' convention)."""
    out = np.empty_like(depth)
    for t in tiles:
        n = t.width * t.height
        inv = np.float32(1.0) / np.maximum(depth[t.offset:t.offset + n], np.float32(0.02))
        out[t.offset:t.offset + n] = (inv - inv.min()) / (inv.max() - inv.min())
    return out


def _scene(lay, seed, out_w, ew):
    tiles, total = O.make_tiles(lay)
    seeds = pf_synth.seeds_for(1, seed)
    gt = pf_synth.scene_depth(seeds, out_w, out_w // 2)[0].numpy()
    base = pf_synth.baseline_emap(seeds, ew, ew // 2)[0].numpy()
    depth = O.warp_depth(gt, tiles, total, O.responses(pf_synth.responses(seeds, lay.ntiles)))
    return tiles, gt, base, _disparity(depth, tiles)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected on a host without a GPU")


def test_mode0_cli_disparity_tiles(tmp_path):
    """C1-size files (512x256 output, 128x64 baseline, 256-wide tiles) in the mode-0 layout,
    tiles in the MiDaS folder convention (--tiles output --ext png)."""
    _need_gpu()
    d = {k: tmp_path / k for k in ("rgb", "gt", "base", "result_hohonet", "output")}
    for p in d.values():
        p.mkdir()
    tw, th = 256, 247
    lay = PL.leres_layout(tw, th)
    tiles, gt, base, disp = _scene(lay, 20261015 + 77, 512, 128)
    raw = "scene01_rgb"
    (d["rgb"] / (raw + ".jpg")).write_bytes(b"\xff\xd8")  # only the name is used
    gq, bq, tq = _q16(gt), _q16(base), _q16(disp)
    _png16_write(d["gt"] / (raw.replace("_rgb", "_depth") + ".png"), gq)
    _png16_write(d["base"] / (raw + ".depth.png"), bq)  # hohonet naming (Main.cpp:512-516)
    for t in range(lay.ntiles):
        f = [_cround(float(v) / MYPI * 180.0) for v in lay.fovs[t]]
        _png16_write(d["output"] / f"{raw}.{f[0]}_{f[1]}_{f[2]}_{f[3]}.png",
                     tq[t * tw * th:(t + 1) * tw * th].reshape(th, tw))
    cmd = [MAIN, "0", str(d["rgb"]), str(d["gt"]), str(d["base"]), str(d["result_hohonet"]),
           "--tiles", str(d["output"]), "--ext", "png", "--width", "512",
           "--tile-model", "disparity"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = _png16_read(d["result_hohonet"] / (raw + ".png"))
    assert got.shape == (256, 512)

    # the binding on the pixels the files decode to
    fz = panofuse.Fuser(0)
    fz.set_tiles(lay)
    t_emap = torch.from_numpy(bq.astype(np.float32) / np.float32(65535.0))[None].to(DEV)
    t_tiles = torch.from_numpy(tq.astype(np.float32) / np.float32(65535.0))[None].to(DEV)
    out = torch.zeros((1, 256, 512), dtype=torch.int16, device=DEV)
    fz.merge_disparity(t_emap.contiguous(), t_tiles.contiguous(), out, ZR)
    fz.synchronize()
    want = out.cpu().numpy().view(np.uint16)[0]
    assert np.array_equal(got, want)

    # without the flag the same files take the cubic model: a different panorama
    (d["result_hohonet"] / (raw + ".png")).unlink()
    r = subprocess.run(cmd[:-2], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out2 = torch.zeros_like(out)
    fz.merge(t_emap.contiguous(), t_tiles.contiguous(), out2, ZR)
    fz.synchronize()
    depth_model = _png16_read(d["result_hohonet"] / (raw + ".png"))
    assert np.array_equal(depth_model, out2.cpu().numpy().view(np.uint16)[0])
    assert not np.array_equal(depth_model, got)

    r = subprocess.run(cmd[:-1] + ["cubic"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "bad --tile-model" in r.stdout


def test_facade_disparity_calls(tmp_path):
    """SolveDisparityToDepth + D2DTransform from C++ equal the binding's register_disparity with
    apply; two active maps are refused."""
    _need_gpu()
    lay = PL.config_layout("C1")
    tiles, _, base, disp = _scene(lay, 31337, 512, 128)
    rng = lay.capped_ranges()
    layout = b"".join(np.asarray(lay.fovs[i], np.float32).tobytes() +
                      np.asarray(rng[i], np.float32).tobytes() for i in range(lay.ntiles))
    blob = (np.array([lay.ntiles, 256, 256], np.int32).tobytes() + layout +
            np.array([128, 64], np.int32).tobytes() + base.astype(np.float32).tobytes() +
            disp.astype(np.float32).tobytes() + np.array(ZR, np.float32).tobytes())
    fi, fo = tmp_path / "in.bin", tmp_path / "out.bin"
    fi.write_bytes(blob)
    r = subprocess.run([CHECK, str(fi), str(fo)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    abcd = np.array([[float.fromhex(v) for v in ln.split()[2:6]]
                     for ln in lines if ln.startswith("abcd ")], np.float32)
    assert abcd.shape == (lay.ntiles, 4)
    assert "two_active 0" in lines
    assert any("exactly one active map" in ln for ln in lines)

    fz = panofuse.Fuser(0)
    fz.set_tiles(lay)
    t_emap = torch.from_numpy(base)[None].to(DEV).contiguous()
    t_tiles = torch.from_numpy(disp)[None].to(DEV).contiguous()
    cf = torch.zeros((1, lay.ntiles, 4), dtype=torch.float32, device=DEV)
    fz.register_disparity(t_emap, t_tiles, ZR, apply=True, coeffs=cf)
    fz.synchronize()
    assert np.array_equal(abcd.view(np.uint32), cf.cpu().numpy()[0].view(np.uint32))
    got = np.fromfile(fo, np.float32)
    assert np.array_equal(got.view(np.uint32), t_tiles.cpu().numpy()[0].view(np.uint32))


def test_facade_exports_the_disparity_symbols():
    r = subprocess.run(["nm", "-DC", DEPTH_LIB], capture_output=True, text=True, check=True)
    exported = [ln for ln in r.stdout.splitlines() if " T " in ln]
    for sym, types in (("DepthNamespace::PerspectiveMap::D2DTransform(", ("Imath::Vec4<float>)",)),
                       ("DepthNamespace::SolveDisparityToDepth(",
                        ("Imath::Vec2<float>&", "Imath::Vec4<float>&")),
                       ("DepthNamespace::MergeDisparityMaps(",
                        ("std::vector<Imath::Vec4<float>", "Imath::Vec2<float>&"))):
        sig = [ln for ln in exported if sym in ln]
        assert len(sig) == 1, sym
        for t in types:
            assert t in sig[0], (sym, sig[0])
