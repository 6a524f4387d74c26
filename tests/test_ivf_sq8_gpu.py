"""The IVF-SQ8 tier (``csrc/kernels/ivf_sq8.hip`` through ``search/sq8.py`` and ``VectorIndex(index_type="ivfsq8")``)
against plain numpy: the code format in float32, bit for bit, and float64 scores ``scale * sum_i q_i c_i`` ordered by
(score descending, list-sorted row ascending) and mapped through ``sorted_ids``."""
import functools

import numpy as np
import pytest
import torch

from bioengine_worker_amd.ops._native import NativeUnavailable
from bioengine_worker_amd.search import sq8
from bioengine_worker_amd.search.index import VectorIndex

pytestmark = pytest.mark.gpu

SIZES = [300, 0, 1, 513, 7, 64, 1200, 2, 0, 900]  # an empty list, one row, more rows than one sweep of a workgroup
PROBES = np.array([[1, 2, 4, 7, 8], [0, 1, 2, 3, 6], [3, 5, 6, 7, 9]])  # 10 (fewer than kk), 2014 and 2679 candidates
N, OFF = sum(SIZES), np.concatenate([[0], np.cumsum(SIZES)])


def _encode(x):
    """The code format in numpy float32: every operation below rounds once to float32, ``rint`` ties to even."""
    x = x.astype(np.float32)
    amax = np.abs(x).max(1)
    inv = np.divide(np.float32(127), amax, out=np.zeros_like(amax), where=amax > 0)
    return np.clip(np.rint(x * inv[:, None]), -127, 127).astype(np.int8), amax / np.float32(127)


def _oracle(q, c, sc, probes, kk):
    """-> per query (rows in order, float64 scores in order, all candidate rows, all their scores)."""
    out = []
    for qi in range(probes.shape[0]):
        rows = np.concatenate([np.arange(OFF[l], OFF[l + 1]) for l in probes[qi]])
        s = sc[rows].astype(np.float64) * (c[rows].astype(np.float64) @ q[qi].astype(np.float64))
        o = np.lexsort((rows, -s))[:kk]
        out.append((rows[o], s[o], rows, s))
    return out


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.mark.parametrize("D", [256, 768, 1024])
def test_encode_exact(gpu, D):
    g = torch.Generator().manual_seed(D)
    src = torch.randn(64, D, generator=g).bfloat16()
    order = torch.randperm(64, generator=g)[:37]
    src[order[0]] = 0  # all zero
    src[order[1]] = 0.3  # equal values
    src[order[2]] = 0
    src[order[2], D - 3] = -1.7  # a single non-zero
    for o in (None, order) if D == 768 else (order,):
        codes, scales = sq8.sq8_encode(src.to(gpu), None if o is None else o.to(gpu))
        c, s = _encode(src.float().numpy() if o is None else src[o].float().numpy())
        assert codes.dtype == torch.int8 and scales.dtype == torch.float32
        assert np.array_equal(codes.cpu().numpy(), c) and np.array_equal(scales.cpu().numpy().view(np.uint32), s.view(np.uint32))
    assert not c[0].any() and s[0] == 0 and (np.abs(c[1]) == 127).all() and np.count_nonzero(c[2]) == 1


@functools.lru_cache(maxsize=None)
def _ints(D):
    """Codes in -4..4 with a few +-127, scales 2^-3..1, queries in -3..3: every partial sum is an integer below
    2^24 and the scale a power of two, so fp32 is exact in any order, and ties are everywhere."""
    rng = np.random.default_rng(D)
    q = rng.integers(-3, 4, (3, D)).astype(np.float32)
    c = rng.integers(-4, 5, (N, D)).astype(np.int8)
    at = rng.integers(0, N * D, 200)
    c.reshape(-1)[at] = np.where(at & 1, 127, -127)
    return q, c, (2.0 ** rng.integers(-3, 1, N)).astype(np.float32), rng.permutation(N).astype(np.int64)


@pytest.mark.parametrize("splits", [1, 3, 7, 64])
@pytest.mark.parametrize("kk", [1, 20, 1024])
@pytest.mark.parametrize("Q", [1, 3])
@pytest.mark.parametrize("D", [256, 768, 1024])
def test_scan_integer_exact(gpu, D, Q, kk, splits):
    q, c, sc, ids = _ints(D)
    S, I = np.full((Q, kk), -np.inf, np.float32), np.full((Q, kk), -1, np.int64)
    for qi, (r, s, _, _) in enumerate(_oracle(q[:Q], c, sc, PROBES[:Q], kk)):
        S[qi, :len(r)], I[qi, :len(r)] = s, ids[r]
    args = (_t(q[:Q], gpu), _t(PROBES[:Q], gpu), _t(OFF, gpu), _t(c, gpu), _t(sc, gpu), _t(ids, gpu), kk)
    s, i = sq8.ivf_sq8_scan_topk_fused(*args, splits=splits)
    s2, i2 = sq8.ivf_sq8_scan_topk_fused(*args, splits=splits)
    assert s.dtype == torch.float32 and i.dtype == torch.int64 and (I[0] == -1).any() == (kk > 10)
    assert np.array_equal(s.cpu().numpy(), S) and np.array_equal(i.cpu().numpy(), I)
    assert torch.equal(s.view(torch.int32), s2.view(torch.int32)) and torch.equal(i, i2)


@pytest.mark.parametrize("kk", [20, 1024])
def test_scan_real_within_rounding(gpu, kk):
    """A returned score is within e = scale D 2^-23 sum_i |q_i c_i| + 2^-24 |score| of the float64 score of its id over
    the dequantised row (twice the first-order bound of a D-term fp32 sum in any order, and the rounding of the one
    multiply by the scale), no row left out beats the last returned one by more than 2 max e, the ids are distinct."""
    D = 768
    g = torch.Generator().manual_seed(kk)
    q = torch.nn.functional.normalize(torch.randn(3, D, generator=g), dim=1).numpy()
    c, sc = _encode(torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=1).bfloat16().float().numpy())
    ids = _ints(D)[3]
    s, i = sq8.ivf_sq8_scan_topk_fused(_t(q, gpu), _t(PROBES, gpu), _t(OFF, gpu), _t(c, gpu), _t(sc, gpu), _t(ids, gpu), kk)
    s, i = s.cpu().numpy().astype(np.float64), i.cpu().numpy()
    row_of = np.argsort(ids)
    for qi, (_, _, rows, ref) in enumerate(_oracle(q, c, sc, PROBES, kk)):
        e = sc[rows] * D * 2.0 ** -23 * (np.abs(c[rows].astype(np.float64)) @ np.abs(q[qi].astype(np.float64)))
        e = e + 2.0 ** -24 * np.abs(ref)
        n = min(kk, len(rows))
        assert (i[qi, n:] == -1).all() and np.isneginf(s[qi, n:]).all() and len(set(i[qi, :n])) == n
        at = np.searchsorted(rows, row_of[i[qi, :n]])  # candidate rows are ascending: PROBES rows are sorted
        assert np.array_equal(rows[at], row_of[i[qi, :n]])
        print(f"q{qi}: largest error / bound {(np.abs(s[qi, :n] - ref[at]) / e[at]).max():.4f}")
        assert (np.abs(s[qi, :n] - ref[at]) <= e[at]).all()
        left = np.setdiff1d(np.arange(len(rows)), at)
        assert (ref[left] <= ref[at].min() + 2 * e.max()).all()


def test_vector_index_sq8(gpu, tmp_path):
    g = torch.Generator().manual_seed(3)
    centers = torch.nn.functional.normalize(torch.randn(40, 768, generator=g), dim=1)
    v = centers[torch.randint(0, 40, (3000,), generator=g)] + 0.5 * torch.randn(3000, 768, generator=g) / 768 ** 0.5
    v = torch.nn.functional.normalize(v, dim=1)
    src = torch.tensor([0, 7, 1500, 2999])
    q = torch.nn.functional.normalize(v[src] + 0.02 * torch.randn(4, 768, generator=g) / 768 ** 0.5, dim=1)
    vi = VectorIndex(dim=768, device=gpu, index_type="ivfsq8", nprobe=8, refine=0)
    vi.add(v)
    nl = vi.centroids.shape[0]
    assert vi.index_type.startswith("IVFSQ8") and vi.lvecs is None
    assert vi.sq_codes.dtype == torch.int8 and vi.sq_codes.shape == (3000, 768) and vi.sq_scales.shape == (3000,)
    # refine = 0: the kernel's scores as they are
    probes = torch.topk((q.to(gpu, vi.dtype) @ vi.centroids.T).float(), 8, dim=1).indices
    s, i = sq8.ivf_sq8_scan_topk_fused(q.to(gpu, vi.dtype).float(), probes, vi.list_off, vi.sq_codes, vi.sq_scales,
                                       vi.sorted_ids, 10)
    S, I = vi.search(q, k=10)
    assert np.array_equal(S.view(np.uint32), s.cpu().numpy().view(np.uint32)) and np.array_equal(I, i.cpu().numpy())
    # refine = 4: the exact top 10 of an IVF-Flat index over the same data
    ref = VectorIndex(dim=768, device=gpu, index_type="ivf", ivf_search="scan")
    ref.add(v)
    vi.refine = 4
    I4 = vi.search(q, k=10, nprobe=nl)[1]
    assert np.array_equal(I4, ref.search(q, k=10, nprobe=nl)[1]) and np.array_equal(I4[:, 0], src.numpy())
    info = vi.save(tmp_path)
    back = VectorIndex.load(tmp_path, device=gpu)
    assert info["sq8"] is True and back.index_type == vi.index_type and back.refine == 4 and back.lvecs is None
    assert torch.equal(back.sq_codes, vi.sq_codes) and torch.equal(back.sq_scales, vi.sq_scales)
    assert np.array_equal(back.search(q, k=10, nprobe=nl)[1], I4)
    back.refine = 0  # the codes' own scores: a function of the rebuilt arrays alone
    for a, b in zip(back.search(q, k=10), (S, I)):
        assert np.array_equal(a, b)
    with pytest.raises(NativeUnavailable):
        vi.search(q, k=1025)
    with pytest.raises(NativeUnavailable):
        VectorIndex(dim=768, device="cpu", index_type="ivfsq8")
    with pytest.raises(NativeUnavailable):
        VectorIndex(dim=384, device=gpu, index_type="ivfsq8")
