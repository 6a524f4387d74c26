"""bench.py --dump-outputs: float32 / float64 ``.npy`` files under one byte budget, and a sample that
depends on the shapes alone, so two runs (or two builds) can be compared element for element."""
import numpy as np
import torch

import bench


def test_dump_outputs_budget_dtypes_and_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4096)
    g = torch.Generator().manual_seed(0)
    outs = {"masks": torch.randint(0, 9, (2, 40, 40), dtype=torch.int32, generator=g),  # 12.8 kB as float32
            "flows": torch.randn(2, 3, 40, 40, generator=g).bfloat16().float(),          # 38.4 kB
            "styles": torch.randn(2, 8, dtype=torch.float64, generator=g)}               # 128 B, kept whole
    bench.dump_outputs(tmp_path / "a", outs)
    bench.dump_outputs(tmp_path / "b", {k: v.clone() for k, v in outs.items()})
    got = {p.stem: np.load(p) for p in (tmp_path / "a").glob("*.npy")}
    assert set(got) == set(outs)
    assert sum(p.stat().st_size for p in (tmp_path / "a").glob("*.npy")) <= 4096 + 3 * 128  # + .npy headers
    assert got["styles"].dtype == np.float64 and np.array_equal(got["styles"], outs["styles"].numpy())
    for name in ("masks", "flows"):
        a = got[name]
        assert a.dtype == np.float32 and a.ndim == 1 and 0 < a.size < outs[name].numel()
        assert np.array_equal(a, np.load(tmp_path / "b" / f"{name}.npy"))
        # every sampled value is an element of the output, taken in flattened order
        flat = outs[name].reshape(-1).float().numpy()
        idx = np.sort(np.random.default_rng(0).choice(flat.size, size=a.size, replace=False))
        assert np.array_equal(a, flat[idx])


def test_dump_outputs_small_outputs_are_written_whole(tmp_path):
    x = torch.arange(24, dtype=torch.int32).reshape(2, 3, 4)
    bench.dump_outputs(tmp_path, {"x": x})
    a = np.load(tmp_path / "x.npy")
    assert a.dtype == np.float32 and a.shape == (2, 3, 4) and np.array_equal(a, x.numpy())
