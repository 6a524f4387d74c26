"""IVF-PQ search kernels (``csrc/kernels/ivfpq_search.hip`` through ``search/ivfpq.py``) against a float64 numpy
oracle: scores from the fp16-rounded table and ``base``, ordered by (score descending, list-sorted row ascending)
and mapped through ``ids``."""
import numpy as np
import pytest
import torch

from bioengine_worker_amd.ops._native import NativeUnavailable
from bioengine_worker_amd.search import ivfpq
from bioengine_worker_amd.search.index import VectorIndex

pytestmark = pytest.mark.gpu

SIZES = [300, 0, 1, 513, 7, 64, 1200, 2, 0, 900]  # an empty list, one row, more rows than a workgroup has threads
PROBES = np.array([[1, 2, 4, 7, 8], [0, 1, 2, 3, 6], [3, 5, 6, 7, 9]])  # 10 (fewer than kk), 2014 and 2679 candidates


def _ints(m, rising, ds=4, seed=0):
    """Queries with one +-1 per sub-space, centroids in -2..2 and codebooks in -4..4: table entries in -4..4 and
    integer scores, ties everywhere.  ``rising``: the score grows with the row (every candidate passes the filter)."""
    rng = np.random.default_rng(seed + m)
    N, off = sum(SIZES), np.concatenate([[0], np.cumsum(SIZES)])
    q = np.zeros((3, m, ds), np.float32)
    cb = rng.integers(-4, 5, (m, 256, ds)).astype(np.float32)
    codes = rng.integers(0, 256, (N, m)).astype(np.uint8)
    base = rng.integers(-3, 4, PROBES.shape).astype(np.float32)
    if rising:
        q[..., 0] = 1
        cb[:] = (np.arange(256) % 9 - 4)[None, :, None]
        level = np.arange(N) * 8 * m // N  # score + 4 m of a row: its first level // 8 codes are 8, the next level % 8
        codes = np.clip(level[:, None] - 8 * np.arange(m)[None], 0, 8).astype(np.uint8)
        base = np.broadcast_to(np.arange(PROBES.shape[1], dtype=np.float32), PROBES.shape).copy()
    else:
        np.put_along_axis(q, rng.integers(0, ds, (3, m, 1)), rng.choice([-1.0, 1.0], (3, m, 1)).astype(np.float32), 2)
    cent = rng.integers(-2, 3, (len(SIZES), m * ds)).astype(np.float32)
    return q.reshape(3, -1), cent, cb, codes, rng.permutation(N).astype(np.int64), off, base


def _lut64(q, cb):
    return np.einsum("qmd,mkd->qmk", q.astype(np.float64).reshape(q.shape[0], cb.shape[0], -1), cb.astype(np.float64))


def _oracle(lut, base, probes, off, codes, kk):
    """-> per query (rows in order, float64 scores in order, all candidate rows, all scores)."""
    out = []
    for qi in range(probes.shape[0]):
        rows = np.concatenate([np.arange(off[l], off[l + 1]) for l in probes[qi]])
        b = np.concatenate([np.full(off[l + 1] - off[l], base[qi, p]) for p, l in enumerate(probes[qi])])
        s = b + lut[qi][np.arange(codes.shape[1])[None], codes[rows]].sum(1)
        o = np.lexsort((rows, -s))[:kk]
        out.append((rows[o], s[o], rows, s))
    return out


def _padded(want, ids, kk):
    S, I = np.full((len(want), kk), -np.inf, np.float32), np.full((len(want), kk), -1, np.int64)
    for qi, (r, s, _, _) in enumerate(want):
        S[qi, :len(r)], I[qi, :len(r)] = s, ids[r]
    return S, I


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.mark.parametrize("rising", [False, True])
@pytest.mark.parametrize("splits", [1, 3, 7, 11])
@pytest.mark.parametrize("kk", [1, 20, 1024])
@pytest.mark.parametrize("Q", [1, 3])
@pytest.mark.parametrize("m", [16, 96, 192])
def test_scan_topk_integer_exact(gpu, m, Q, kk, splits, rising):
    q, _, cb, codes, ids, off, base = _ints(m, rising)
    lut, probes, base = _lut64(q, cb)[:Q], PROBES[:Q], base[:Q]
    S, I = _padded(_oracle(lut, base, probes, off, codes, kk), ids, kk)
    args = (_t(lut, gpu).half(), _t(base, gpu), _t(probes, gpu), _t(off, gpu), _t(codes, gpu), _t(ids, gpu), kk)
    s, i = ivfpq.ivfpq_scan_topk_fused(*args, splits=splits)
    s2, i2 = ivfpq.ivfpq_scan_topk_fused(*args, splits=splits)
    assert s.dtype == torch.float32 and i.dtype == torch.int64 and (I[0] == -1).any() == (kk > 10)
    assert np.array_equal(s.cpu().numpy(), S) and np.array_equal(i.cpu().numpy(), I)
    assert torch.equal(s.view(torch.int32), s2.view(torch.int32)) and torch.equal(i, i2)


@pytest.mark.parametrize("m, kk, splits", [(96, 20, None), (192, 1024, 3), (16, 100, 7)])
def test_scan_topk_real_within_rounding(gpu, m, kk, splits):
    """A returned score is within e = m 2^-23 (|base| + sum_j |t_j|) of the float64 score of its id (twice the
    first-order bound of an m-term fp32 chain), and no row is left out that beats the last returned one by 2 e."""
    _, _, _, codes, ids, off, _ = _ints(m, False)
    g = torch.Generator().manual_seed(m)
    q = torch.nn.functional.normalize(torch.randn(3, m * 4, generator=g), dim=1)
    cb = 0.05 * torch.randn(m, 256, 4, generator=g)
    base = torch.randn(PROBES.shape, generator=g)
    lut = ivfpq.ivfpq_lut_fused(q.to(gpu), cb.to(gpu))
    s, i = ivfpq.ivfpq_scan_topk_fused(lut, base.to(gpu), _t(PROBES, gpu), _t(off, gpu), _t(codes, gpu), _t(ids, gpu), kk,
                                       splits=splits)
    s, i, lut64 = s.cpu().numpy().astype(np.float64), i.cpu().numpy(), lut.cpu().numpy().astype(np.float64)
    row_of = np.argsort(ids)
    for qi, (_, _, rows, sc) in enumerate(_oracle(lut64, base.numpy().astype(np.float64), PROBES, off, codes, kk)):
        mag = np.concatenate([np.full(off[l + 1] - off[l], abs(float(base[qi, p]))) for p, l in enumerate(PROBES[qi])])
        e = m * 2.0 ** -23 * (mag + np.abs(lut64[qi][np.arange(m)[None], codes[rows]]).sum(1))
        n = min(kk, len(rows))
        assert (i[qi, n:] == -1).all() and np.isneginf(s[qi, n:]).all() and len(set(i[qi, :n])) == n
        at = np.searchsorted(rows, row_of[i[qi, :n]])  # candidate rows are ascending here: PROBES rows are sorted
        assert np.array_equal(rows[at], row_of[i[qi, :n]])
        print(f"q{qi}: largest error / bound {(np.abs(s[qi, :n] - sc[at]) / e[at]).max():.3f}")
        assert (np.abs(s[qi, :n] - sc[at]) <= e[at]).all()
        left = np.setdiff1d(np.arange(len(rows)), at)
        assert (sc[left] <= sc[at].min() + 2 * e.max()).all()


@pytest.mark.parametrize("ds", [4, 8])
def test_lut(gpu, ds):
    """Exact on integers; on real data within 2^-11 |exact| + 2^-25 + ds 2^-24 sum_i |q_i c_i| (fp16 rounding, its
    subnormal step, the fp32 chain)."""
    rng = np.random.default_rng(ds)
    q, cb = rng.integers(-3, 4, (5, 16 * ds)).astype(np.float32), rng.integers(-4, 5, (16, 256, ds)).astype(np.float32)
    got = ivfpq.ivfpq_lut_fused(_t(q, gpu), _t(cb, gpu))
    assert got.dtype == torch.float16 and np.array_equal(got.cpu().numpy().astype(np.float64), _lut64(q, cb))
    q, cb = rng.standard_normal((5, 16 * ds)).astype(np.float32), rng.standard_normal((16, 256, ds)).astype(np.float32)
    got = ivfpq.ivfpq_lut_fused(_t(q, gpu), _t(cb, gpu)).cpu().numpy().astype(np.float64)
    want, mag = _lut64(q, cb), _lut64(np.abs(q), np.abs(cb))
    assert (np.abs(got - want) <= 2.0 ** -11 * np.abs(want) + 2.0 ** -25 + ds * 2.0 ** -24 * mag).all()


@pytest.mark.parametrize("search", ["scan", "fused"])
def test_index_search_integer_exact(gpu, search):
    m, kk = 96, 20
    q, cent, cb, codes, ids, off, _ = _ints(m, False, seed=1)
    idx = ivfpq.IVFPQIndex(dim=4 * m, nlist=len(SIZES), m=m, nprobe=len(SIZES), device=gpu, search=search)
    idx.centroids, idx.codebooks, idx.codes, idx.ids, idx.list_off = (_t(a, gpu) for a in (cent, cb, codes, ids, off))
    probes = np.tile(np.arange(len(SIZES)), (3, 1))
    S, I = _padded(_oracle(_lut64(q, cb), q.astype(np.float64) @ cent.T, probes, off, codes, kk), ids, kk)
    s, i = idx.search(q, kk)
    assert np.array_equal(s, S)
    if search == "fused":
        assert np.array_equal(i, I)
        sd, idv = idx.search_device(_t(q, gpu), kk)
        assert sd.is_cuda and np.array_equal(sd.cpu().numpy(), S) and np.array_equal(idv.cpu().numpy(), I)
        with pytest.raises(NativeUnavailable):
            idx.search(q, 1025)


def test_vector_index_fused_search(gpu):
    g = torch.Generator().manual_seed(3)
    centers = torch.nn.functional.normalize(torch.randn(40, 768, generator=g), dim=1)
    v = centers[torch.randint(0, 40, (3000,), generator=g)] + 0.5 * torch.randn(3000, 768, generator=g) / 768 ** 0.5
    v = torch.nn.functional.normalize(v, dim=1)
    q = torch.nn.functional.normalize(v[:1] + 0.02 * torch.randn(1, 768, generator=g) / 768 ** 0.5, dim=1)
    vi = VectorIndex(dim=768, device=gpu, index_type="ivfpq", pq_search="fused")
    vi.add(v)
    assert vi.pq.search_mode == "fused" and vi.pq.fused_search(1, 5)
    for refine in (4, 0):
        vi.refine = refine
        assert vi.search(q, k=5)[1][0, 0] == 0
    with pytest.raises(NativeUnavailable):
        ivfpq.IVFPQIndex(dim=768, nlist=3, m=96, device="cpu", search="fused")
