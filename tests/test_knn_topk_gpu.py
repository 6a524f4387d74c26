"""Fused neighbour tables on the GPU (``csrc/kernels/knn_topk.hip`` through ``search/umap.py``): the coarse
kernel exactly on integer data, both tables against the float64 oracle, and the fallback of uncertified rows."""
import numpy as np
import pytest
import torch

import umap_cases as uc
import umap_transform_cases as tc
from bioengine_worker_amd.search import reference as ref
from bioengine_worker_amd.search import umap as gu

pytestmark = pytest.mark.gpu


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.mark.parametrize("m, n, K, kk, S, self_base", [
    (1, 70, 32, 5, 1, -1),          # a single row, one ragged tile
    (37, 131, 64, 20, 1, 0),        # two tiles, the second 3 columns wide; the fit's self column
    (130, 1000, 96, 64, 3, -1),     # two row blocks, a half K step, kk = 64, splits of 2 / 3 / 3 tiles
    (70, 333, 2304, 31, 3, 11),     # 36 K steps, one tile per split, a shifted self column
    (5, 40, 32, 64, 1, -1),         # fewer columns than kk: -inf / -1 padding
    (9, 300, 32, 1, 2, -1),         # kk = 1
])
def test_topk_integer_exact(gpu, m, n, K, kk, S, self_base):
    """Entries in -3..3: every product and partial sum is an integer below 2^24, so fp32 is exact, ties are
    everywhere, and the lists must equal a stable argsort of the negated scores bit for bit."""
    rng = np.random.default_rng(m * 1000 + n)
    A = rng.integers(-3, 4, (m, K)).astype(np.float32)
    B = rng.integers(-3, 4, (n, K)).astype(np.float32)
    s = (A.astype(np.float64) @ B.astype(np.float64).T)
    if self_base >= 0:
        s[np.arange(m), self_base + np.arange(m)] = -np.inf
    order = np.argsort(-s, axis=1, kind="stable")[:, :kk]
    want_s = np.take_along_axis(s, order, 1)
    want_i = np.where(np.isfinite(want_s), order, -1)
    if n < kk:
        want_s = np.concatenate([want_s, np.full((m, kk - n), -np.inf)], 1)
        want_i = np.concatenate([want_i, np.full((m, kk - n), -1)], 1)
    gs, gi = gu.knn_topk_bf16(_t(A, gpu).bfloat16(), _t(B, gpu).bfloat16(), kk, self_base, splits=S)
    assert gs.shape == (m, kk) and gi.dtype == torch.int32
    assert np.array_equal(gi.cpu().numpy(), want_i)
    assert np.array_equal(gs.cpu().numpy().astype(np.float64), want_s)


@pytest.mark.parametrize("n, d, k", [(131, 8, 5), (300, 32, 15)])
def test_fused_table(gpu, n, d, k):
    """Bound as ``test_umap_gpu.test_knn_table``: (d + 8) 2^-23.  The certificate cannot fail on these sets (the
    gap to the first non-candidate is 0.143 / 0.038 against an eps below 5e-5)."""
    x = uc.tie_free(n, d, k)
    idx, dist = ref.knn_table(x, k)
    gi, gd = gu.knn_table_gpu(_t(x, gpu), k, method="fused", splits=3)
    ti, _ = gu.knn_table_gpu(_t(x, gpu), k, method="torch")
    err = np.abs(gd.cpu().numpy().astype(np.float64) - dist).max()
    print(f"fused kNN n={n}: largest distance error {err:.3e}, fallback rows {gi.knn_fallback_rows}")
    assert gi.knn_method == "fused" and gi.knn_fallback_rows == 0
    assert np.array_equal(gi.cpu().numpy(), idx) and torch.equal(gi, ti)
    assert err <= (d + 8) * 2.0 ** -23


@pytest.mark.parametrize("name", ["q131", "c300"])
def test_fused_query_table(gpu, name):
    c = tc.case(name)
    q, x, k, d = _t(c["q"], gpu), _t(c["x"], gpu), c["k"], c["x"].shape[1]
    gi, gd = gu.knn_query_table_gpu(q, x, k, method="fused", splits=2)
    ti, _ = gu.knn_query_table_gpu(q, x, k, method="torch")
    err = np.abs(gd.cpu().numpy().astype(np.float64) - c["dist"]).max()
    print(f"fused query table {name}: largest distance error {err:.3e}, fallback rows {gi.knn_fallback_rows}")
    assert gi.knn_method == "fused" and gi.knn_fallback_rows == 0
    assert np.array_equal(gi.cpu().numpy(), c["idx"]) and torch.equal(gi, ti)
    assert err <= (d + 8) * 2.0 ** -23


def test_fused_table_fallback(gpu):
    """40 copies of one point among 200: a copy's 20 candidates tie with the 19 copies left out, so its row cannot
    be certified and is recomputed by the torch rule.  Indices among exact ties are not compared."""
    n, d, k = 200, 16, 5
    x = np.random.default_rng(40).standard_normal((n, d)).astype(np.float32)
    dup = np.arange(3, n, 5)
    x[dup] = x[3]
    gi, gd = gu.knn_table_gpu(_t(x, gpu), k, method="fused")
    gi_h, gd_h = gi.cpu().numpy(), gd.cpu().numpy().astype(np.float64)
    xn = x.astype(np.float64) / np.sqrt((x.astype(np.float64) ** 2).sum(1))[:, None]
    exact = np.take_along_axis(np.maximum(0, 1 - xn @ xn.T), gi_h.astype(np.int64), 1)
    exact[:, 0] = 0.0
    print(f"fallback rows {gi.knn_fallback_rows} of {n}, largest distance error {np.abs(gd_h - exact).max():.3e}")
    assert dup.size == 40 and 40 <= gi.knn_fallback_rows < n
    assert np.array_equal(gi_h[:, 0], np.arange(n))
    assert np.abs(gd_h - exact).max() <= (d + 8) * 2.0 ** -23
    assert np.isin(gi_h[dup], dup).all() and gd_h[dup].max() <= (d + 8) * 2.0 ** -23
    assert all(len(set(r)) == k for r in gi_h.tolist())
