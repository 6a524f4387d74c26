"""The flat tier's fused search (``csrc/kernels/flat_scan_topk.hip`` through ``search/flat.py`` and ``VectorIndex``)
against a float64 numpy oracle: ``v.astype(float64) @ q``, ordered by (score descending, row ascending)."""
import functools
import itertools

import numpy as np
import pytest
import torch

from bioengine_worker_amd.ops._native import NativeUnavailable
from bioengine_worker_amd.search.flat import FLAT_MAX_K, flat_scan_topk_fused
from bioengine_worker_amd.search.index import VectorIndex

pytestmark = pytest.mark.gpu

# the first value of an axis is the base case.  N: below one fragment, a partial fragment, a partial 64-row block,
# 20 tiles of 256 rows over ranges that do not divide them; Q: one lane column, a full tile, a partial second tile, a
# full group, the split into two groups; splits: 64 leaves ranges empty; rising: every list overflows repeatedly
AXES = {"N": [5003, 1, 17, 64 * 3 + 5], "Q": [17, 1, 16, 64, 65], "kk": [20, 1, 64, FLAT_MAX_K],
        "splits": [3, 1, 7, 64], "D": [768, 32, 1024], "rising": [False, True]}
# axes that meet in the code: the group rule (Q, kk, D), empty ranges and padding (N, splits, kk), overflow (rising)
PAIRS = [("Q", "kk"), ("Q", "D"), ("kk", "D"), ("N", "splits"), ("N", "kk"), ("rising", "kk"), ("rising", "Q")]


def _cases():
    base = {a: v[0] for a, v in AXES.items()}
    out = [base] + [{**base, a: x} for a, v in AXES.items() for x in v[1:]]
    out += [{**base, a: x, b: y} for a, b in PAIRS for x, y in itertools.product(AXES[a][1:], AXES[b][1:])]
    return [tuple(c.values()) for c in out]


@functools.lru_cache(maxsize=None)
def _ints(D, rising):
    """Rows in -4..4, queries in -3..3 (exact in bf16): every partial sum is an integer below 2^24, so the MFMA's fp32
    accumulation is exact in any order, and ties are everywhere.  ``rising``: the score grows with the row."""
    rng = np.random.default_rng(D)
    n = max(AXES["N"])
    q = rng.integers(-3, 4, (max(AXES["Q"]), D)).astype(np.float32)
    v = rng.integers(-4, 5, (n, D)).astype(np.float32)
    if rising:
        q[:] = 1
        v = (np.clip((np.arange(n) * 8 * D // n)[:, None] - 8 * np.arange(D)[None], 0, 8) - 4).astype(np.float32)
    return q, v


def _oracle(q, v, kk):
    """-> scores [Q, kk] float64 and rows [Q, kk], padded with -inf / -1."""
    S, I = np.full((len(q), kk), -np.inf), np.full((len(q), kk), -1, np.int64)
    for qi in range(len(q)):
        s = v.astype(np.float64) @ q[qi].astype(np.float64)
        o = np.lexsort((np.arange(len(v)), -s))[:kk]
        S[qi, :len(o)], I[qi, :len(o)] = s[o], o
    return S, I


def _bf(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev).bfloat16()


@pytest.mark.parametrize("N,Q,kk,splits,D,rising", _cases())
def test_flat_scan_integer_exact(gpu, N, Q, kk, splits, D, rising):
    q, v = _ints(D, rising)
    q, v = q[:Q], v[:N]
    S, I = _oracle(q, v, kk)
    args = (_bf(q, gpu), _bf(v, gpu), kk)
    s, i = flat_scan_topk_fused(*args, splits=splits)
    s2, i2 = flat_scan_topk_fused(*args, splits=splits)
    assert s.dtype == torch.float32 and i.dtype == torch.int64 and (I[0] == -1).any() == (kk > N)
    assert np.array_equal(s.cpu().numpy(), S.astype(np.float32)) and np.array_equal(i.cpu().numpy(), I)
    assert torch.equal(s.view(torch.int32), s2.view(torch.int32)) and torch.equal(i, i2)


@pytest.mark.parametrize("kk", [20, FLAT_MAX_K])
def test_flat_scan_real_within_rounding(gpu, kk):
    """A returned score is within e = D 2^-23 sum_i |q_i v_i| of the float64 score of its row over the bf16-rounded
    operands (twice the first-order bound of a D-term fp32 sum in any order), no row left out beats the last
    returned one by more than 2 e, and the ids are distinct."""
    D, N = 768, 5003
    g = torch.Generator().manual_seed(kk)
    q = torch.nn.functional.normalize(torch.randn(3, D, generator=g), dim=1).bfloat16()
    v = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=1).bfloat16()
    s, i = flat_scan_topk_fused(q.to(gpu), v.to(gpu), kk)
    s, i = s.cpu().numpy().astype(np.float64), i.cpu().numpy()
    q64, v64 = q.float().numpy().astype(np.float64), v.float().numpy().astype(np.float64)
    for qi in range(3):
        sc, e = v64 @ q64[qi], D * 2.0 ** -23 * (np.abs(v64) @ np.abs(q64[qi]))
        at = i[qi]
        assert len(set(at)) == kk and at.min() >= 0 and at.max() < N
        print(f"q{qi}: largest error / bound {(np.abs(s[qi] - sc[at]) / e[at]).max():.4f}")
        assert (np.abs(s[qi] - sc[at]) <= e[at]).all()
        left = np.setdiff1d(np.arange(N), at)
        assert (sc[left] <= sc[at].min() + 2 * e.max()).all()


def test_vector_index_fused_against_gemm(gpu, tmp_path):
    q, v = _ints(768, False)
    q, v = q[:5], v[:3000]
    vi = VectorIndex(dim=768, device=gpu, index_type="flat", flat_search="gemm")
    vi.add(v)
    got = {}
    for mode in ("gemm", "fused"):
        vi.flat_search = mode
        assert vi.fused_flat_search(5, 10) == (mode == "fused")
        got[mode] = vi.search(q, k=10)
    S, I = _oracle(q, v, 10)
    assert np.array_equal(got["gemm"][0].view(np.uint32), got["fused"][0].view(np.uint32))
    assert np.array_equal(got["fused"][0], S.astype(np.float32)) and np.array_equal(got["fused"][1], I)
    with pytest.raises(NativeUnavailable):
        vi.search(q, k=FLAT_MAX_K + 1)
    with pytest.raises(NativeUnavailable):
        VectorIndex(dim=768, device="cpu", flat_search="fused")
    vi.save(tmp_path)
    back = VectorIndex.load(tmp_path, device=gpu, flat_search="fused")
    assert back.fused_flat_search(5, 10) and np.array_equal(back.search(q, k=10)[1], I)
