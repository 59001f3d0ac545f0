"""bench.py --dump-outputs on the CPU: bench.dump_outputs writes float32 arrays of the u16 result
(int16 storage), stays inside its byte budget, samples the same positions in every run, and
--sample-dump is refused without --full.  The GPU side (the plain line and the files of a real
run) is in tests/test_gpu_bench_pipeline.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import bench  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _result(seed, shape):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-32768, 32768, shape, dtype=torch.int16, generator=g)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_small_result_is_written_whole(tmp_path):
    out, co = _result(1, (3, 8, 16)), torch.randn(3, 5, 4)
    bench.dump_outputs(str(tmp_path), out, co, 0, 1)
    z = _load(tmp_path)
    assert set(z) == {"coeffs", "fused", "fused_sample"}
    assert all(a.dtype == np.float32 for a in z.values())
    u16 = out.numpy().view(np.uint16).astype(np.float32)  # 0..65535, never negative
    assert np.array_equal(z["fused"], u16) and np.array_equal(z["fused_sample"], u16.ravel())
    assert np.array_equal(z["coeffs"], co.numpy())


def test_large_result_is_sampled_within_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET", 4 * 4000)  # 4000 float32 elements in all
    out, co = _result(2, (7, 20, 37)), torch.randn(7, 5, 4)  # 5180 px, 740 per panorama
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), out, co, 0, 1)
    bench.dump_outputs(str(b), out, co, 0, 1)
    za, zb = _load(a), _load(b)
    assert sum(v.size for v in za.values()) <= 4000
    u16 = out.numpy().view(np.uint16).astype(np.float32)
    assert np.array_equal(za["fused"], u16[:2])  # the leading panoramas that fit half the budget
    assert za["fused_sample"].size == 2000 - co.numel()
    assert all(np.array_equal(za[k], zb[k]) for k in za)  # same positions, run to run
    # the sample reaches past the panoramas written whole
    other = _result(3, (7, 20, 37))
    other[:2] = out[:2]
    bench.dump_outputs(str(tmp_path / "c"), other, co, 0, 1)
    assert not np.array_equal(_load(tmp_path / "c")["fused_sample"], za["fused_sample"])


def test_ranks_share_the_budget_and_name_their_files(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET", 4 * 4000)
    out, co = _result(4, (7, 20, 37)), torch.randn(7, 5, 4)
    bench.dump_outputs(str(tmp_path), out, co, 1, 2)
    z = _load(tmp_path)
    assert set(z) == {"coeffs_rank1", "fused_rank1", "fused_sample_rank1"}
    assert sum(v.size for v in z.values()) <= 2000


def test_sample_dump_needs_full(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--sample-dump",
                        str(tmp_path / "s")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--full" in r.stderr and not r.stdout.strip()
