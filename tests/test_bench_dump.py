"""bench.py --dump-outputs: the arrays stay within the byte budget, small ones whole, large ones as a seeded sample."""
import os

import numpy as np
import torch

import bench


def test_dump_outputs_budget_and_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 1 << 20)
    g = torch.Generator().manual_seed(0)
    named = [("small", torch.randn((1000,), generator=g)), ("big", torch.randn((4, 200_000), generator=g)),
             ("half", torch.randn((50, 100), generator=g, dtype=torch.float64))]
    a, b = tmp_path / "a", tmp_path / "b"
    info = bench.dump_outputs(str(a), named)
    assert bench.dump_outputs(str(b), named) == info
    total = sum(os.path.getsize(a / f) for f in os.listdir(a))
    assert total <= bench.DUMP_BUDGET_BYTES
    assert sorted(os.listdir(a)) == ["big.npy", "half.npy", "small.npy"]
    for name, t in named:
        got = np.load(a / f"{name}.npy")
        assert got.dtype == np.float32
        assert np.array_equal(got, np.load(b / f"{name}.npy"))
        assert info[name]["shape"] == list(t.shape)
    assert not info["small"]["sampled"] and np.array_equal(np.load(a / "small.npy"), named[0][1].numpy())
    assert np.array_equal(np.load(a / "half.npy"), named[2][1].float().numpy())
    big = np.load(a / "big.npy")
    assert info["big"]["sampled"] and big.ndim == 1 and 0 < big.size < 800_000
    assert np.isin(big, named[1][1].numpy().reshape(-1)).all()
