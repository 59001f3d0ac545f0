"""The general (scalar) form of the streamed Jacobi passes against the packed form.

The general form runs where a level lacks the separable-coverage certificate, and under PF_JSLOW;
no layout of the suite lacks the certificate, so nothing else runs it.  One C2 panorama, the
level-0 kernel switched to streamed passes so that all three levels stream: this process fuses
with the packed form, a fresh child process (PF_JSLOW is read once per process) fuses the same
inputs with PF_JSLOW=1, and the two u16 panoramas must be equal bit for bit.  The child's PF_JPLAN
lines must say `general` for every level, so the test cannot pass by taking the packed form twice.
"""
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

DEV = "cuda:0"
W, H = 2048, 1024


def _fuse(emap, tiles, coeffs):
    """The C2 fusion of one panorama with every level streamed; the u16 panorama as numpy."""
    f = panofuse.Fuser(0)
    try:
        f.set_tiles(PL.config_layout("C2"))
        f.set_jacobi_engine(resident=False)
        out = torch.zeros((1, H, W), dtype=torch.int16, device=DEV)
        f.fuse(emap, tiles, out, PL.ZENITH_RANGE, coeffs=coeffs)
        torch.cuda.synchronize()
        return out.cpu().numpy().view(np.uint16)
    finally:
        f.close()


def _child(inputs_path, out_path):
    z = np.load(inputs_path)
    emap, tiles, coeffs = (torch.from_numpy(z[k]).to(DEV).contiguous()
                           for k in ("emap", "tiles", "coeffs"))
    _fuse(emap, tiles, coeffs).tofile(out_path)


CHILD = ("import sys; sys.path[:0] = [{pkg!r}, {tests!r}]; "
         "import test_gpu_jacobi_general as t; t._child(sys.argv[1], sys.argv[2])")


def test_general_form_matches_packed(tmp_path):
    lay = PL.config_layout("C2")
    seeds = pf_synth.seeds_for(1, 20261019 + 7)
    gt = pf_synth.scene_depth(seeds, W, H, DEV).contiguous()
    emap = pf_synth.baseline_emap(seeds, 512, 256, DEV).contiguous()
    f = panofuse.Fuser(0)
    try:
        f.set_tiles(lay)
        tiles = torch.zeros((1, f.tile_elems), dtype=torch.float32, device=DEV)
        f.warp_depth(gt, tiles, panofuse.make_responses(pf_synth.responses(seeds, lay.ntiles), DEV))
        coeffs = torch.zeros((1, lay.ntiles, 4), dtype=torch.float32, device=DEV)
        f.register(emap, tiles, PL.ZENITH_RANGE, apply=False, coeffs=coeffs)
        torch.cuda.synchronize()
    finally:
        f.close()
    packed = _fuse(emap, tiles, coeffs)

    inputs_path, out_path = tmp_path / "inputs.npz", tmp_path / "general.u16"
    np.savez(inputs_path, emap=emap.cpu().numpy(), tiles=tiles.cpu().numpy(),
             coeffs=coeffs.cpu().numpy())
    env = dict(os.environ, PF_JSLOW="1", PF_JPLAN="1")
    code = CHILD.format(pkg=os.path.dirname(os.path.abspath(panofuse.__file__)),
                        tests=os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code, str(inputs_path), str(out_path)], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]

    plans = [ln for ln in r.stderr.splitlines() if ln.startswith("jacobi plan")]
    assert len(plans) == 3, r.stderr[-2000:]
    for ln, w in zip(plans, (512, 1024, 2048)):
        assert ln.startswith(f"jacobi plan {w}x") and " general C2:" in ln, ln

    general = np.fromfile(out_path, dtype=np.uint16).reshape(packed.shape)
    bad = int((general != packed).sum())
    assert bad == 0, f"{bad} pixels of the general form differ from the packed form's"
    assert np.count_nonzero(packed) > 0
