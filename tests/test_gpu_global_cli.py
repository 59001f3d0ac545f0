"""GPU end-to-end of the global alignment above the C-ABI: the mode-0 command line with
--global-align, and the facade's SolveDepthToDepth2 / TransformResult / MedianScaling /
CopyInvalidPixels called from compiled C++ (tests/cpp/global_link.cpp).  Both are held to the
binding and to the CPU restatement (tests/global_ref.py)."""
import math
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import global_ref as G  # noqa: E402
import panofuse  # noqa: E402
import pf_layouts as PL  # noqa: E402
import pf_synth  # noqa: E402
import pyoracle as O  # noqa: E402

PKG = os.path.dirname(os.path.dirname(panofuse.LIB_PATH))
MAIN = os.path.join(PKG, "bin", "panofuse_main")
LINK = os.path.join(PKG, "bin", "pf_global_link")
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


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected on a host without a GPU")


def test_mode0_cli_global_align(tmp_path):
    """C1-size files (512x256 output, 128x64 baseline, 256-wide tiles) in the mode-0 layout."""
    _need_gpu()
    d = {k: tmp_path / k for k in ("rgb", "gt", "base", "result_hohonet", "tiles")}
    for p in d.values():
        p.mkdir()
    tw, th = 256, 247
    lay = PL.leres_layout(tw, th)
    tiles, total = O.make_tiles(lay)
    seeds = pf_synth.seeds_for(1, 20261019 + 5)
    gt = pf_synth.scene_depth(seeds, 512, 256)[0].numpy()
    base = pf_synth.baseline_emap(seeds, 128, 64)[0].numpy()
    depth = O.warp_depth(gt, tiles, total, O.responses(pf_synth.responses(seeds, lay.ntiles)))
    raw = "scene01_rgb"
    (d["rgb"] / (raw + ".jpg")).write_bytes(b"\xff\xd8")  # only the name is used
    gq, bq, tq = _q16(gt), _q16(base), _q16(depth)
    _png16_write(d["gt"] / (raw.replace("_rgb", "_depth") + ".png"), gq)
    _png16_write(d["base"] / (raw + ".depth.png"), bq)  # hohonet naming (Main.cpp:512-516)
    for t in range(lay.ntiles):
        f = [_cround(float(v) / MYPI * 180.0) for v in lay.fovs[t]]
        _png16_write(d["tiles"] / f"{raw}.{f[0]}_{f[1]}_{f[2]}_{f[3]}.png",
                     tq[t * tw * th:(t + 1) * tw * th].reshape(th, tw))
    cmd = [MAIN, "0", str(d["rgb"]), str(d["gt"]), str(d["base"]), str(d["result_hohonet"]),
           "--tiles", str(d["tiles"]), "--ext", "png", "--width", "512"]
    env = {k: v for k, v in os.environ.items() if k != "PF_GLOBAL_ALIGN"}
    r = subprocess.run(cmd + ["--global-align"], capture_output=True, text=True, timeout=120,
                       env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    got = _png16_read(d["result_hohonet"] / (raw + ".png"))
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("[SolveDepthToDepth2] abcd:(")]
    assert len(line) == 1 and " cost:" in line[0] and "->" in line[0], r.stdout
    aligned_txt = (d["result_hohonet"] / (raw + ".aligned.txt")).read_text()

    # the binding on the pixels the files decode to
    fz = panofuse.Fuser(0)
    fz.set_tiles(lay)
    base_f = bq.astype(np.float32) / np.float32(65535.0)
    t_emap = torch.from_numpy(base_f)[None].to(DEV).contiguous()
    t_tiles = torch.from_numpy(tq.astype(np.float32) / np.float32(65535.0))[None].to(DEV)
    plain = torch.zeros((1, 256, 512), dtype=torch.int16, device=DEV)
    fz.merge(t_emap, t_tiles.contiguous(), plain, ZR)
    aligned = plain.clone()
    cf = torch.zeros((1, 4), dtype=torch.float32, device=DEV)
    fz.register_global(t_emap, aligned, ZR, apply=True, coeffs=cf)
    fz.synchronize()
    plain = plain.cpu().numpy().view(np.uint16)[0]
    aligned = aligned.cpu().numpy().view(np.uint16)[0]
    assert np.array_equal(got, aligned)
    assert not np.array_equal(aligned, plain)
    # and the restatement on the binding's merge
    _, abcd, _ = G.register_global(base_f, plain, ZR)
    assert np.array_equal(cf.cpu().numpy()[0].view(np.uint32), abcd.view(np.uint32))
    assert np.array_equal(aligned, G.result_transform(plain, ZR, abcd))
    # the metrics are taken on the aligned result
    vals = dict(ln.split(": ") for ln in aligned_txt.strip().splitlines())
    gt_f = gq.astype(np.float32) / np.float32(65535.0)
    ref = O.error_metrics(gt_f, aligned, ZR, 1, True)
    ref_plain = O.error_metrics(gt_f, plain, ZR, 1, True)
    assert abs(float(vals["mae_result"]) - ref["mae"]) <= 5.01e-7
    assert abs(ref["mae"] - ref_plain["mae"]) > 1e-5  # the two results do score differently

    # without the flag: the plain merge
    for f in d["result_hohonet"].iterdir():
        f.unlink()
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "[SolveDepthToDepth2]" not in r.stdout
    assert np.array_equal(_png16_read(d["result_hohonet"] / (raw + ".png")), plain)


def _fill(w, h, scale, bias):
    """tests/cpp/global_link.cpp's fill(): bias + scale * (float)((i * 37) % 101) / 101.0f."""
    i = np.arange(w * h, dtype=np.int64)
    k = ((i * 37) % 101).astype(np.float32)
    v = (np.float32(scale) * k).astype(np.float32) / np.float32(101.0)
    return (np.float32(bias) + v.astype(np.float32)).astype(np.float32).reshape(h, w)


def test_facade_calls_from_cpp():
    _need_gpu()
    r = subprocess.run([LINK, "gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = {ln.split()[0]: ln.split()[1:] for ln in r.stdout.splitlines() if ln and ln[0].isupper()}
    emap = _fill(16, 8, 0.6, 0.2)
    i = np.arange(64 * 32, dtype=np.int64)
    data = (4000 + (i * 131) % 50000).astype(np.uint16).reshape(32, 64)
    _, abcd, s = G.register_global(emap, data, ZR)
    got = np.array([np.float32(v) for v in out["ABCD"]], np.float32)
    assert np.array_equal(got.view(np.uint32), abcd.view(np.uint32))
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("[SolveDepthToDepth2]")][0]
    assert line == (f"[SolveDepthToDepth2] abcd:({abcd[0]:.6g} {abcd[1]:.6g} {abcd[2]:.6g} "
                    f"{abcd[3]:.6g}) cost:{s['initial_cost']:.6g}->{s['final_cost']:.6g}")
    want = G.result_transform(data, ZR, abcd)
    acc = 0
    for v in want.reshape(-1).tolist():
        acc = (acc * 1315423911 + v) & 0xFFFFFFFFFFFFFFFF
    assert int(out["BAND"][0]) == acc
    a, b = _fill(20, 10, 0.9, 0.0), _fill(16, 8, 0.4, 0.1)
    b.reshape(-1)[7], b.reshape(-1)[9] = 0.0, 1.0
    ok, m0, m1, scaled = G.median_scale(a, b)
    assert out["MED"][0] == "1" and ok
    assert np.float32(out["MED"][1]) == m0 and np.float32(out["MED"][2]) == m1
    masked = G.copy_invalid(scaled, b)
    assert int(out["MASK"][0]) == int((masked != scaled).sum()) > 0
