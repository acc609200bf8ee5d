"""bench.py --dump-outputs DIR without a GPU: what the timed step handed its caller is written as float32 .npy files, large arrays as fixed seeded
samples, 64 MB at most in all (tests/test_gpu_bench_cli.py runs the benchmark itself)."""
import os, sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _fake_trainer(seed, n_out, n_w):
    g = torch.Generator().manual_seed(seed)
    return SimpleNamespace(last_outs=torch.randn(n_out, generator=g).to(torch.bfloat16), flat=torch.randn(n_w, generator=g))


def test_dump_outputs_writes_float32_samples(tmp_path):
    import bench
    tr = _fake_trainer(0, 8 * 4 * 352 * 352, 3_000_000)
    loss = torch.tensor([1.0, 2.0, 3.0, 4.0, 10.0])
    bench.dump_outputs(str(tmp_path / "a"), tr, loss)
    bench.dump_outputs(str(tmp_path / "b"), tr, loss)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["logits.npy", "loss.npy", "weights.npy"]
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float32 and np.array_equal(a, b)          # the same arrays give the same sample, run after run
        total += os.path.getsize(tmp_path / "a" / n)
    assert total <= 64 << 20
    assert np.array_equal(np.load(tmp_path / "a" / "loss.npy"), loss.numpy())
    w = np.load(tmp_path / "a" / "weights.npy")
    assert w.shape == (bench.DUMP_SAMPLE,) and np.isin(w, tr.flat.numpy()).all()       # sampled elements, not a reduction
    lg = np.load(tmp_path / "a" / "logits.npy")
    assert lg.shape == (bench.DUMP_SAMPLE,) and np.isin(lg, tr.last_outs.float().numpy()).all()


def test_dump_outputs_small_arrays_whole_and_no_logits_without_maps(tmp_path):
    import bench
    tr = SimpleNamespace(last_outs=None, flat=torch.arange(1000, dtype=torch.float32))
    bench.dump_outputs(str(tmp_path), tr, torch.zeros(5))
    assert sorted(os.listdir(tmp_path)) == ["loss.npy", "weights.npy"]
    assert np.array_equal(np.load(tmp_path / "weights.npy"), np.arange(1000, dtype=np.float32))

