"""IVF-PQ coarse quantizer (``csrc/kernels/coarse_assign.hip`` through ``search/ivfpq.py``) against a float64 numpy
oracle: the raw top-2 kernel bit for bit on data whose scores are exact in fp32, the certificate on real data, clear
and ambiguous rows, and the path through ``IVFPQIndex`` / ``VectorIndex``."""
import numpy as np
import pytest
import torch

from bioengine_worker_amd.ops._native import NativeUnavailable
from bioengine_worker_amd.search import ivfpq
from bioengine_worker_amd.search.index import VectorIndex

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16


def _data(kind, n, nlist, D, seed=0):
    """float32 ``x [n, D]`` and centroids ``[nlist, D]`` (all values exact in the row dtype the case uses).
    ``ints``: small integers, ties everywhere.  ``xlo`` / ``clo``: ``i + j 2^-10`` with i, j in -3..3 on the x / the
    centroid side (``hi`` and ``lo`` both exact in bf16, the other side integer: every score is a multiple of 2^-10
    below 2^14, exact in fp32).  ``unit``: normalised Gaussian rows."""
    rng = np.random.default_rng(seed + 7 * n + 3 * nlist + D)
    if kind == "unit":
        x, c = rng.standard_normal((n, D)), rng.standard_normal((nlist, D))
        x, c = x / np.linalg.norm(x, axis=1, keepdims=True), c / np.linalg.norm(c, axis=1, keepdims=True)
        return x.astype(np.float32), c.astype(np.float32)
    a, b = (1, 1) if D == 64 else (3, 2)
    x = rng.integers(-a, a + 1, (n, D)).astype(np.float32)
    c = rng.integers(-b, b + 1, (nlist, D)).astype(np.float32)
    if kind == "xlo":
        x = (rng.integers(-3, 4, (n, D)) + rng.integers(-3, 4, (n, D)) * 2.0 ** -10).astype(np.float32)
    if kind == "clo":
        c = (rng.integers(-3, 4, (nlist, D)) + rng.integers(-3, 4, (nlist, D)) * 2.0 ** -10).astype(np.float32)
    return x, c


def _oracle(x, c):
    """float64 scores ``[n, nlist]`` and per row (i1, s1, s2) under (score descending, index ascending)."""
    s = x.astype(np.float64) @ c.astype(np.float64).T
    order = np.argsort(-s, axis=1, kind="stable")
    rows = np.arange(s.shape[0])
    s2 = s[rows, order[:, 1]] if s.shape[1] > 1 else np.full(s.shape[0], -np.inf)
    return s, order[:, 0], s[rows, order[:, 0]], s2


def _certified(x, c, eps):
    """The rows ``coarse_assign_fused`` certifies, by its own rule on the raw kernel's output."""
    _, s1, s2 = ivfpq.coarse_top2_fused(x, c)
    bound = torch.linalg.vector_norm(x, dim=1, dtype=F32) * torch.linalg.vector_norm(c.float(), dim=1).max() * (2 * eps)
    return (s1 - s2 > bound).cpu().numpy()


@pytest.mark.parametrize("kind, n, nlist, D, dtype", [
    ("ints", 1, 1, 64, F32), ("ints", 130, 3, 64, BF16), ("ints", 257, 255, 768, BF16), ("ints", 513, 257, 768, F32),
    ("ints", 257, 700, 64, F32), ("ints", 513, 1, 768, BF16), ("xlo", 130, 257, 768, F32), ("xlo", 257, 3, 64, F32),
    ("clo", 513, 700, 768, BF16), ("clo", 1, 255, 64, BF16), ("clo", 130, 700, 64, F32)])
def test_top2_exact(gpu, kind, n, nlist, D, dtype):
    x, c = _data(kind, n, nlist, D)
    _, i1, s1, s2 = _oracle(x, c)
    gi, g1, g2 = ivfpq.coarse_top2_fused(torch.from_numpy(x).to(gpu, dtype), torch.from_numpy(c).to(gpu))
    assert gi.dtype == torch.int32 and gi.shape == g1.shape == g2.shape == (n,)
    assert np.array_equal(gi.cpu().numpy(), i1)
    assert np.array_equal(g1.cpu().numpy().view(np.uint32), s1.astype(np.float32).view(np.uint32))
    assert np.array_equal(g2.cpu().numpy().view(np.uint32), s2.astype(np.float32).view(np.uint32))


@pytest.mark.parametrize("xs, cs, dtype", [(1.0, 1.0, F32), (1.0, 1.0, BF16), (3.0, 0.5, F32)])
def test_certificate_real(gpu, xs, cs, dtype):
    x, c = _data("unit", 513, 300, 768)
    xt, ct = (xs * torch.from_numpy(x)).to(gpu, dtype), (cs * torch.from_numpy(c)).to(gpu)
    eps = ivfpq.coarse_certificate_eps(768, 2 if dtype == BF16 else 3)
    assign, fallback = ivfpq.coarse_assign_fused(xt, ct)
    cert = _certified(xt, ct, eps)
    x64, c64 = xt.float().cpu().numpy().astype(np.float64), ct.cpu().numpy().astype(np.float64)
    s, i1, s1, _ = _oracle(x64, c64)
    a = assign.cpu().numpy()
    slack = 2 * eps * np.linalg.norm(x64, axis=1) * np.linalg.norm(c64, axis=1).max()
    print(f"eps {eps:.3e}, fallback rows {fallback} of 513, rows that differ from the oracle {int((a != i1).sum())}")
    assert assign.dtype == torch.int64 and fallback == int((~cert).sum())
    assert np.array_equal(a[cert], i1[cert])
    assert (s1 - s[np.arange(513), a] <= slack).all()
    assert fallback <= 513 // 4


@pytest.mark.parametrize("dup", [False, True])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_clear_and_duplicate_rows(gpu, dtype, dup):
    _, c = _data("unit", 1, 300, 768)
    noise, _ = _data("unit", 513, 1, 768, seed=1)
    want = np.arange(513) % 300
    if dup:  # rows nearest to the pair tie exactly: they fall back, and the torch rule gives the smaller index
        c[7] = c[2]
    x = c[want] + 0.05 * noise
    xt = torch.from_numpy(x / np.linalg.norm(x, axis=1, keepdims=True)).to(gpu, dtype)
    assign, fallback = ivfpq.coarse_assign_fused(xt, torch.from_numpy(c).to(gpu))
    assert fallback == (int(np.isin(want, (2, 7)).sum()) if dup else 0)
    assert np.array_equal(assign.cpu().numpy(), np.where(dup & (want == 7), 2, want))


def _clustered(n, seed):
    g = torch.Generator().manual_seed(seed)
    centers = torch.nn.functional.normalize(torch.randn(40, 768, generator=g), dim=1)
    v = centers[torch.randint(0, 40, (n,), generator=g)] + 0.5 * torch.randn(n, 768, generator=g) / 768 ** 0.5
    return torch.nn.functional.normalize(v, dim=1)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_index_fused_coarse(gpu, dtype):
    v = _clustered(3000, 4).to(gpu)
    idx = ivfpq.IVFPQIndex(dim=768, nlist=64, m=96, device=gpu, build="fused", coarse="fused")
    idx.train(v)
    trained = idx.coarse_fallback_rows
    rows = v.to(dtype)
    idx.add(rows)
    cert = _certified(rows, idx.centroids, ivfpq.coarse_certificate_eps(768, 2 if dtype == BF16 else 3))
    a = idx._assign.cpu().numpy()
    _, i1, _, _ = _oracle(rows.float().cpu().numpy(), idx.centroids.cpu().numpy())
    assert np.array_equal(a[cert], i1[cert])
    assert idx.coarse_fallback_rows - trained == int((~cert).sum()) and trained >= 0
    assert np.array_equal(idx.list_off.cpu().numpy(), np.concatenate([[0], np.cumsum(np.bincount(a, minlength=64))]))
    _, ids = idx.search(v[:8], k=5)
    assert all(i in ids[i] for i in range(8))


def test_vector_index_fused_coarse(gpu):
    v = _clustered(3000, 3)
    vi = VectorIndex(dim=768, device=gpu, index_type="ivfpq", pq_coarse="fused")
    vi.add(v)
    assert vi.pq is not None and vi.pq.coarse == "fused" and vi.pq.fused_coarse(vi.pq.nlist)
    assert vi.pq.ntotal == 3000 and vi.pq.coarse_fallback_rows >= 0
    _, ids = vi.search(v[:4], k=5)
    assert np.array_equal(ids[:, 0], np.arange(4))


def test_coarse_argument():
    with pytest.raises(NativeUnavailable):
        ivfpq.IVFPQIndex(dim=768, nlist=64, m=96, device="cpu", coarse="fused")
    with pytest.raises(ValueError):
        ivfpq.IVFPQIndex(dim=768, nlist=64, m=96, device="cpu", coarse="mfma")
