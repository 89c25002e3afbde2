"""CPU tier: bench.py --dump-outputs (bench.dump_outputs) on a stand-in engine: the files it writes, their dtypes,
the 64 MB limit and that the gradient sample sits at the same positions from run to run."""
import types

import numpy as np
import pytest
import torch

import bench


def _engine(n16, n32, seed=0):
    g = torch.Generator().manual_seed(seed)
    return types.SimpleNamespace(
        logits=torch.randn(4, 10, generator=g).half(),
        flat16=torch.randn(n16, generator=g).half(), flat32=torch.randn(n32, generator=g),
        gflat16=torch.randn(n16, generator=g).half(), gflat32=torch.randn(n32, generator=g))


def test_dump_outputs_files_dtypes_and_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_GRAD_SAMPLE", 1000)
    e = _engine(5003, 777)
    bench.dump_outputs(tmp_path / "a", e, 2.5)
    bench.dump_outputs(tmp_path / "b", e, 2.5)
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == ["grads_fp16.npy", "grads_fp32.npy", "logits.npy", "loss.npy", "weights_fp16.npy",
                     "weights_fp32.npy"]
    a = {n: np.load(tmp_path / "a" / n) for n in names}
    for n in names:
        assert a[n].dtype in (np.float32, np.float64), n
        assert np.array_equal(a[n], np.load(tmp_path / "b" / n)), n
    assert a["loss.npy"].tolist() == [2.5]
    assert np.array_equal(a["logits.npy"], e.logits.float().numpy())
    assert np.array_equal(a["weights_fp16.npy"], e.flat16.float().numpy())
    assert np.array_equal(a["weights_fp32.npy"], e.flat32.numpy())
    # the sample: 1000 distinct positions of the larger buffer in ascending order, the whole of the smaller one
    idx = np.sort(np.random.default_rng(0).choice(5003, size=1000, replace=False))
    assert np.array_equal(a["grads_fp16.npy"], e.gflat16.float().numpy()[idx])
    assert np.array_equal(a["grads_fp32.npy"], e.gflat32.numpy())


def test_dump_outputs_refuses_more_than_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4 * 5000)
    with pytest.raises(AssertionError):
        bench.dump_outputs(tmp_path, _engine(5003, 777), 0.0)
    assert not list(tmp_path.glob("*.npy"))
