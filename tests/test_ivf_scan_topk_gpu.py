"""IVF-Flat search with the top-k inside the scan (``csrc/kernels/ivf_scan_topk.hip`` through ``search/index.py``)
against a float64 numpy oracle: exact inner products with the bf16 rows, ordered by (score descending, list-sorted
row ascending) and mapped through ``sorted_ids``; and against the existing scan kernel, bit for bit."""
import functools

import numpy as np
import pytest
import torch

from bioengine_worker_amd.ops._native import NativeUnavailable
from bioengine_worker_amd.search import index
from bioengine_worker_amd.search.index import VectorIndex

pytestmark = pytest.mark.gpu

SIZES = [300, 0, 1, 513, 7, 64, 1200, 2, 0, 900]  # an empty list, one row, more rows than one sweep of a workgroup
PROBES = np.array([[1, 2, 4, 7, 8], [0, 1, 2, 3, 6], [3, 5, 6, 7, 9]])  # 10 (fewer than kk), 2014 and 2679 candidates
N, OFF = sum(SIZES), np.concatenate([[0], np.cumsum(SIZES)])


@functools.lru_cache(maxsize=None)
def _ints(D, rising):
    """Rows in -4..4 (exact in bf16), queries in -3..3: every partial sum is an integer below 2^24, so fp32 is exact
    in any order, and ties are everywhere.  ``rising``: the score grows with the row (every candidate passes)."""
    rng = np.random.default_rng(D)
    q = rng.integers(-3, 4, (3, D)).astype(np.float32)
    v = rng.integers(-4, 5, (N, D)).astype(np.float32)
    if rising:
        q[:] = 1
        v = (np.clip((np.arange(N) * 8 * D // N)[:, None] - 8 * np.arange(D)[None], 0, 8) - 4).astype(np.float32)
    return q, v, rng.permutation(N).astype(np.int64)


def _oracle(q, v, probes, kk):
    """-> per query (rows in order, float64 scores in order, all candidate rows, all their scores)."""
    out = []
    for qi in range(probes.shape[0]):
        rows = np.concatenate([np.arange(OFF[l], OFF[l + 1]) for l in probes[qi]])
        s = v[rows].astype(np.float64) @ q[qi].astype(np.float64)
        o = np.lexsort((rows, -s))[:kk]
        out.append((rows[o], s[o], rows, s))
    return out


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.mark.parametrize("rising", [False, True])
@pytest.mark.parametrize("splits", [1, 3, 7, 64])
@pytest.mark.parametrize("kk", [1, 20, 1024])
@pytest.mark.parametrize("Q", [1, 3])
@pytest.mark.parametrize("D", [128, 768, 1024])
def test_scan_topk_integer_exact(gpu, D, Q, kk, splits, rising):
    q, v, ids = _ints(D, rising)
    S, I = np.full((Q, kk), -np.inf, np.float32), np.full((Q, kk), -1, np.int64)
    for qi, (r, s, _, _) in enumerate(_oracle(q[:Q], v, PROBES[:Q], kk)):
        S[qi, :len(r)], I[qi, :len(r)] = s, ids[r]
    args = (_t(q[:Q], gpu), _t(PROBES[:Q], gpu), _t(OFF, gpu), _t(v, gpu).bfloat16(), _t(ids, gpu), kk)
    s, i = index.ivf_scan_topk_fused(*args, splits=splits)
    s2, i2 = index.ivf_scan_topk_fused(*args, splits=splits)
    assert s.dtype == torch.float32 and i.dtype == torch.int64 and (I[0] == -1).any() == (kk > 10)
    assert np.array_equal(s.cpu().numpy(), S) and np.array_equal(i.cpu().numpy(), I)
    assert torch.equal(s.view(torch.int32), s2.view(torch.int32)) and torch.equal(i, i2)


@pytest.mark.parametrize("kk", [20, 1024])
def test_scan_topk_real_within_rounding(gpu, kk):
    """A returned score is within e = D 2^-23 sum_i |q_i v_i| of the float64 score of its id over the bf16-rounded
    row (twice the first-order bound of a D-term fp32 sum in any order), no row left out beats the last returned
    one by more than 2 e, and the ids are distinct."""
    D = 768
    g = torch.Generator().manual_seed(kk)
    q = torch.nn.functional.normalize(torch.randn(3, D, generator=g), dim=1)
    v = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=1).bfloat16()
    ids = _ints(D, False)[2]
    s, i = index.ivf_scan_topk_fused(q.to(gpu), _t(PROBES, gpu), _t(OFF, gpu), v.to(gpu), _t(ids, gpu), kk)
    s, i, q64, v64 = s.cpu().numpy().astype(np.float64), i.cpu().numpy(), q.numpy(), v.float().numpy()
    row_of = np.argsort(ids)
    for qi, (_, _, rows, sc) in enumerate(_oracle(q64, v64, PROBES, kk)):
        e = D * 2.0 ** -23 * (np.abs(v64[rows].astype(np.float64)) @ np.abs(q64[qi].astype(np.float64)))
        n = min(kk, len(rows))
        assert (i[qi, n:] == -1).all() and np.isneginf(s[qi, n:]).all() and len(set(i[qi, :n])) == n
        at = np.searchsorted(rows, row_of[i[qi, :n]])  # candidate rows are ascending: PROBES rows are sorted
        assert np.array_equal(rows[at], row_of[i[qi, :n]])
        print(f"q{qi}: largest error / bound {(np.abs(s[qi, :n] - sc[at]) / e[at]).max():.4f}")
        assert (np.abs(s[qi, :n] - sc[at]) <= e[at]).all()
        left = np.setdiff1d(np.arange(len(rows)), at)
        assert (sc[left] <= sc[at].min() + 2 * e.max()).all()


def test_vector_index_fused_against_scan(gpu):
    g = torch.Generator().manual_seed(3)
    centers = torch.nn.functional.normalize(torch.randn(40, 768, generator=g), dim=1)
    v = centers[torch.randint(0, 40, (3000,), generator=g)] + 0.5 * torch.randn(3000, 768, generator=g) / 768 ** 0.5
    v = torch.nn.functional.normalize(v, dim=1)
    src = torch.tensor([0, 7, 1500, 2999])
    q = torch.nn.functional.normalize(v[src] + 0.02 * torch.randn(4, 768, generator=g) / 768 ** 0.5, dim=1)
    vi = VectorIndex(dim=768, device=gpu, index_type="ivf", nprobe=8, ivf_search="scan")
    vi.add(v)
    got = {}
    for mode in ("scan", "fused"):
        vi.ivf_search = mode
        assert vi.fused_ivf_search(4, 10) == (mode == "fused")
        got[mode] = vi.search(q, k=10)[0]
        assert np.array_equal(vi.search(q, k=10, nprobe=vi.centroids.shape[0])[1][:, 0], src.numpy())
    assert np.array_equal(got["scan"].view(np.uint32), got["fused"].view(np.uint32))
    with pytest.raises(NativeUnavailable):
        vi.search(q, k=1025)
    with pytest.raises(NativeUnavailable):
        VectorIndex(dim=768, device="cpu", ivf_search="fused")
