"""IVF-PQ build kernels (``csrc/kernels/pq_build.hip`` through ``search/ivfpq.py``) against a float64 numpy oracle:
the fused residual encoding exactly on integer data and within the fp32 rounding bound on real data, one k-means
step of the codebooks, and the path through ``IVFPQIndex`` / ``VectorIndex``."""
import numpy as np
import pytest
import torch

from bioengine_worker_amd.ops._native import NativeUnavailable
from bioengine_worker_amd.search import ivfpq
from bioengine_worker_amd.search.index import VectorIndex

pytestmark = pytest.mark.gpu


def _ints(n, D, m, seed=0):
    """x in -3..3, three coarse centroids in -2..2, codebooks in -4..4, an assignment that uses every list:
    all distances are integers below 300, exact in fp32 (and x in bf16), with ties in ~8 % of the minima."""
    rng = np.random.default_rng(seed + n + D + m)
    x = rng.integers(-3, 4, (n, D)).astype(np.float32)
    c = rng.integers(-2, 3, (3, D)).astype(np.float32)
    cb = rng.integers(-4, 5, (m, 256, D // m)).astype(np.float32)
    a = rng.integers(0, 3, n).astype(np.int32)
    a[:3] = np.arange(3)[:n]
    return x, c, a, cb


def _dist(r, cb):
    """float64 ``|cb_k|^2 - 2 r.cb_k`` [n, m, 256]; np.argmin over the last axis takes the first minimum."""
    cb = cb.astype(np.float64)
    rs = r.astype(np.float64).reshape(r.shape[0], cb.shape[0], -1)
    return (cb ** 2).sum(-1)[None] - 2 * np.einsum("nmd,mkd->nmk", rs, cb)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n", [1, 130, 257])
@pytest.mark.parametrize("D, m", [(768, 96), (768, 192), (64, 16)])
def test_encode_integer_exact(gpu, D, m, n, dtype):
    x, c, a, cb = _ints(n, D, m)
    want = _dist(x - c[a], cb).argmin(-1)
    got = ivfpq.pq_encode_fused(_t(x, gpu).to(dtype), _t(c, gpu), _t(a, gpu), _t(cb, gpu))
    assert got.dtype == torch.uint8 and got.shape == (n, m)
    assert np.array_equal(got.cpu().numpy(), want)


def test_encode_real_within_rounding(gpu):
    """The chosen codeword's float64 distance may exceed the minimum by the rounding of two fp32 scores of at
    most ds + 1 operations each: (ds + 2) 2^-23 max_k(|cb_k|^2 + 2 sum_i |r_i cb_k,i|)."""
    D, m, n, ds = 768, 96, 257, 8
    g = torch.Generator().manual_seed(5)
    x = torch.nn.functional.normalize(torch.randn(n, D, generator=g), dim=1)
    c = torch.nn.functional.normalize(torch.randn(3, D, generator=g), dim=1)
    a = (x @ c.T).argmax(1).int()
    r = x - c[a.long()]  # the fp32 residual, on both sides
    cb = ivfpq._pq_train(r, m, 3, g)
    got = ivfpq.pq_encode_fused(x.to(gpu), c.to(gpu), a.to(gpu), cb.to(gpu)).cpu().numpy().astype(np.int64)
    d = _dist(r.numpy(), cb.numpy())
    cb64, rs = cb.numpy().astype(np.float64), np.abs(r.numpy().astype(np.float64)).reshape(n, m, ds)
    mag = ((cb64 ** 2).sum(-1)[None] + 2 * np.einsum("nmd,mkd->nmk", rs, np.abs(cb64))).max(-1)
    excess = np.take_along_axis(d, got[..., None], -1)[..., 0] - d.min(-1)
    print(f"largest excess / bound {(excess / ((ds + 2) * 2.0 ** -23 * mag)).max():.3f}, "
          f"codes equal to the oracle's {np.mean(got == d.argmin(-1)):.4f}")
    assert (excess <= (ds + 2) * 2.0 ** -23 * mag).all()


@pytest.mark.parametrize("S", [257, 1000])
@pytest.mark.parametrize("D, m", [(768, 96), (64, 16)])
def test_kmeans_step_integer_exact(gpu, D, m, S):
    x, c, a, cb = _ints(S, D, m, seed=1)
    res = x - c[a]
    cb[:, 255] = 100.0  # far from every residual: its count is 0
    codes = _dist(res, cb).argmin(-1)  # [S, m]
    rs = res.astype(np.float64).reshape(S, m, -1)
    want, cnt = np.zeros(cb.shape), np.zeros((m, 256))
    for j in range(m):
        np.add.at(want[j], codes[:, j], rs[:, j])
        np.add.at(cnt[j], codes[:, j], 1)
    want /= np.maximum(cnt, 1)[..., None]
    new = ivfpq.pq_kmeans_step_fused(_t(res, gpu), _t(cb, gpu))
    again = ivfpq.pq_kmeans_step_fused(_t(res, gpu), _t(cb, gpu))
    got = new.cpu().numpy()
    used = cnt > 0
    assert not used[:, 255].any() and used.any(1).all()
    assert (np.abs(got[used].astype(np.float64) - want[used]) <= 2.0 ** -23 * np.abs(want[used])).all()
    assert np.array_equal(got[~used].view(np.uint32), cb[~used].view(np.uint32))
    assert torch.equal(new.view(torch.int32), again.view(torch.int32))


def test_index_fused_build(gpu):
    n, D, m = 257, 768, 96
    x, c, _, cb = _ints(n, D, m, seed=2)
    idx = ivfpq.IVFPQIndex(dim=D, nlist=3, m=m, device=gpu, build="fused")
    idx.centroids, idx.codebooks = _t(c, gpu), _t(cb, gpu)
    idx.add(_t(x, gpu).bfloat16())
    a = idx._assign.cpu().numpy()
    assert np.array_equal(idx._raw().cpu().numpy(), _dist(x - c[a], cb).argmin(-1))
    assert np.array_equal(idx.list_off.cpu().numpy(), np.concatenate([[0], np.cumsum(np.bincount(a, minlength=3))]))
    with pytest.raises(NativeUnavailable):
        ivfpq.IVFPQIndex(dim=D, nlist=3, m=m, device="cpu", build="fused")


def test_vector_index_fused_build(gpu):
    g = torch.Generator().manual_seed(3)
    centers = torch.nn.functional.normalize(torch.randn(40, 768, generator=g), dim=1)
    v = centers[torch.randint(0, 40, (3000,), generator=g)] + 0.5 * torch.randn(3000, 768, generator=g) / 768 ** 0.5
    v = torch.nn.functional.normalize(v, dim=1)
    q = torch.nn.functional.normalize(v[:1] + 0.02 * torch.randn(1, 768, generator=g) / 768 ** 0.5, dim=1)
    vi = VectorIndex(dim=768, device=gpu, index_type="ivfpq", pq_build="fused")
    vi.add(v)
    assert vi.pq is not None and vi.pq.build == "fused" and vi.pq.fused_build
    _, ids = vi.search(q, k=5)
    assert ids[0, 0] == 0
