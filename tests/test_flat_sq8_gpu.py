"""The flat SQ8 tier (``csrc/kernels/flat_sq8_scan_topk.hip`` through ``search/flat.py`` and
``VectorIndex(index_type="flatsq8")``) against plain numpy: the query split and the score contract in float32, bit for
bit, ordered by (score descending, row ascending)."""
import functools
import itertools
import json

import numpy as np
import pytest
import torch

from bioengine_worker_amd.ops._native import NativeUnavailable
from bioengine_worker_amd.search.flat import FLAT_SQ8_MAX_K, flat_sq8_scan_topk_fused
from bioengine_worker_amd.search.index import VectorIndex
from bioengine_worker_amd.search.sq8 import sq8_encode

pytestmark = pytest.mark.gpu

# the first value of an axis is the base case.  N: below one fragment, a partial fragment, a partial 64-row block, 20
# tiles of 256 rows over ranges that do not divide them; Q: one lane column, a full fragment, a partial second one, a
# full group, the split into two groups; splits: 64 leaves ranges empty; data: "l0" has l = 0 in every query (ties
# everywhere), "rising" scores that grow with the row (every list overflows repeatedly)
AXES = {"N": [5003, 1, 17, 64 * 3 + 5], "Q": [17, 1, 16, 32, 33], "kk": [20, 1, 64, FLAT_SQ8_MAX_K],
        "splits": [3, 1, 7, 64], "D": [768, 256, 1024], "data": ["mixed", "l0", "rising"]}
# axes that meet in the code: the group rule and the LDS (Q, kk, D), empty ranges and padding (N, splits, kk), overflow
PAIRS = [("Q", "kk"), ("Q", "D"), ("kk", "D"), ("N", "splits"), ("N", "kk"), ("data", "kk"), ("data", "Q")]


def _cases():
    base = {a: v[0] for a, v in AXES.items()}
    out = [base] + [{**base, a: x} for a, v in AXES.items() for x in v[1:]]
    out += [{**base, a: x, b: y} for a, b in PAIRS for x, y in itertools.product(AXES[a][1:], AXES[b][1:])]
    return [tuple(c.values()) for c in out]


def _split(q):
    """The query rule in numpy float32 -> (h, l, sq): every operation rounds once to float32, ``rint`` ties to even."""
    q = q.astype(np.float32)
    amax = np.abs(q).max(1)
    inv = np.divide(np.float32(127), amax, out=np.zeros_like(amax), where=amax > 0)
    t = q * inv[:, None]
    h = np.clip(np.rint(t), -127, 127)
    return h, np.clip(np.rint((t - h) * np.float32(256)), -127, 127), amax / np.float32(127)


def _scores32(q, c, sc):
    """The score contract in numpy float32 -> [Q, N].  H and L are exact in float64 (integers below 2^53)."""
    h, l, sq = _split(q)
    c = c.astype(np.float64)
    H, L = (h.astype(np.float64) @ c.T).astype(np.float32), (l.astype(np.float64) @ c.T).astype(np.float32)
    return (sc[None] * sq[:, None]) * (H + L * np.float32(2.0 ** -8))


def _topk(S, kk):
    """Scores [Q, N] -> the first kk of each query under (score descending, row ascending), padded with -inf / -1."""
    out_s, out_i = np.full((len(S), kk), -np.inf, S.dtype), np.full((len(S), kk), -1, np.int64)
    for qi, s in enumerate(S):
        o = np.lexsort((np.arange(len(s)), -s))[:kk]
        out_s[qi, :len(o)], out_i[qi, :len(o)] = s[o], o
    return out_s, out_i


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@functools.lru_cache(maxsize=None)
def _ints(D, data):
    """Codes in -4..4 with a few +-127, power-of-two scales, queries (h + l / 256) 2^e with h in -3..3, l in -127..127
    and one element h = 127, l = 0: amax = 127 2^e, inv = 2^-e, the split recovers h and l, |H| < 2^15 and H + L / 256
    fits 23 bits, so the float64 product scale * sq * (H + L / 256) is the kernel's fp32 score exactly."""
    rng = np.random.default_rng(D)
    n, nq = max(AXES["N"]), max(AXES["Q"])
    h, l = rng.integers(-3, 4, (nq, D)), rng.integers(-127, 128, (nq, D))
    c = rng.integers(-4, 5, (n, D))
    at = rng.integers(0, n * D, 200)
    c.reshape(-1)[at] = np.where(at & 1, 127, -127)
    sc = 2.0 ** rng.integers(-3, 1, n)
    if data != "mixed":
        l[:] = 0
    if data == "rising":
        h[:] = 1
        c = np.clip((np.arange(n) * 8 * D // n)[:, None] - 8 * np.arange(D)[None], 0, 8) - 4
        sc[:] = 1
    top = rng.integers(0, D, nq)
    h[np.arange(nq), top], l[np.arange(nq), top] = 127, 0
    q = (h + l / 256.0) * 2.0 ** rng.integers(-2, 3, nq)[:, None]
    return q.astype(np.float32), c.astype(np.int8), sc.astype(np.float32)


@pytest.mark.parametrize("N,Q,kk,splits,D,data", _cases())
def test_flat_sq8_integer_exact(gpu, N, Q, kk, splits, D, data):
    q, c, sc = _ints(D, data)
    q, c, sc = q[:Q], c[:N], sc[:N]
    h, l, sq = _split(q)
    t = (h.astype(np.float64) @ c.astype(np.float64).T) + (l.astype(np.float64) @ c.astype(np.float64).T) / 256
    S, I = _topk(sc[None].astype(np.float64) * sq[:, None] * t, kk)  # the float64 oracle
    args = (_t(q, gpu), _t(c, gpu), _t(sc, gpu), kk)
    s, i = flat_sq8_scan_topk_fused(*args, splits=splits)
    s2, i2 = flat_sq8_scan_topk_fused(*args, splits=splits)
    assert s.dtype == torch.float32 and i.dtype == torch.int64 and (I[0] == -1).any() == (kk > N)
    assert np.array_equal(s.cpu().numpy(), S.astype(np.float32)) and np.array_equal(i.cpu().numpy(), I)
    assert torch.equal(s.view(torch.int32), s2.view(torch.int32)) and torch.equal(i, i2)


def test_flat_sq8_saturated(gpu):
    """D = 1024, every code 127 against h = 127, l = 0: H = 16 516 096 = D 127^2 survives int32 -> fp32."""
    q, c = np.ones((2, 1024), np.float32), np.full((300, 1024), 127, np.int8)
    sc = (2.0 ** -(np.arange(300) % 4)).astype(np.float32)
    S, I = _topk(_scores32(q, c, sc), 20)
    assert S.max() == np.float32(1) / np.float32(127) * np.float32(16516096)
    s, i = flat_sq8_scan_topk_fused(_t(q, gpu), _t(c, gpu), _t(sc, gpu), 20)
    assert np.array_equal(s.cpu().numpy().view(np.uint32), S.view(np.uint32)) and np.array_equal(i.cpu().numpy(), I)


@pytest.mark.parametrize("kk", [20, FLAT_SQ8_MAX_K])
def test_flat_sq8_real_bit_equal(gpu, kk):
    """Unit-norm rows (encoded by ``sq8_encode``) and queries: every returned score is bit-equal to the float32
    contract of its row, no row with a better key is left out, and the ids are distinct: the result is the float32
    oracle's list."""
    g = torch.Generator().manual_seed(kk)
    q = torch.nn.functional.normalize(torch.randn(3, 768, generator=g), dim=1)
    v = torch.nn.functional.normalize(torch.randn(5003, 768, generator=g), dim=1).bfloat16()
    c, sc = sq8_encode(v.to(gpu))
    s, i = flat_sq8_scan_topk_fused(q.to(gpu), c, sc, kk)
    S, I = _topk(_scores32(q.numpy(), c.cpu().numpy(), sc.cpu().numpy()), kk)
    i = i.cpu().numpy()
    assert all(len(set(r)) == kk for r in i) and np.array_equal(i, I)
    assert np.array_equal(s.cpu().numpy().view(np.uint32), S.view(np.uint32))


def test_vector_index_flat_sq8(gpu, tmp_path):
    """3000 random unit rows (cosines below 0.2) and, per query, k = 10 planted rows at cosines 0.60, 0.59 .. 0.51.
    The SQ8 score error is at most (amax / 254) |q|_1 <= (amax / 254) sqrt(D), about 0.015 here, so the planted rows
    cannot leave a shortlist of 4 k, and the 0.01 steps dwarf the fp32 re-rank error."""
    D, k, g = 768, 10, torch.Generator().manual_seed(5)
    unit = lambda x: torch.nn.functional.normalize(x, dim=1)  # noqa: E731
    q, v = unit(torch.randn(3, D, generator=g)), unit(torch.randn(3000, D, generator=g))
    for qi in range(3):
        u = torch.randn(k, D, generator=g)
        u = unit(u - (u @ q[qi])[:, None] * q[qi])
        cos = 0.60 - 0.01 * torch.arange(k)[:, None]
        v[100 + 900 * qi:100 + 900 * qi + k] = cos * q[qi] + (1 - cos ** 2).sqrt() * u
    vi = VectorIndex(dim=D, device=gpu, index_type="flatsq8", refine=0)
    vi.add(v)
    assert vi.index_type == "FlatSQ8-GPU" and vi.centroids is None
    assert vi.sq_codes.dtype == torch.int8 and vi.sq_codes.shape == (3000, D) and vi.sq_scales.shape == (3000,)
    two = VectorIndex(dim=D, device=gpu, index_type="flatsq8")
    two.add(v[:1100])
    two.add(v[1100:])
    assert torch.equal(two.sq_codes, vi.sq_codes) and torch.equal(two.sq_scales, vi.sq_scales)
    # refine = 0: the wrapper's result on the bf16-rounded queries
    s, i = flat_sq8_scan_topk_fused(q.to(gpu).bfloat16().float(), vi.sq_codes, vi.sq_scales, k)
    S0, I0 = vi.search(q, k=k)
    assert np.array_equal(S0.view(np.uint32), s.cpu().numpy().view(np.uint32)) and np.array_equal(I0, i.cpu().numpy())
    # refine = 4: the float64 oracle's ids on the bf16-rounded rows and queries
    ref = _topk(q.bfloat16().double().numpy() @ v.bfloat16().double().numpy().T, k)[1]
    assert np.array_equal(ref, 100 + 900 * np.arange(3)[:, None] + np.arange(k)[None])
    vi.refine = 4
    I4 = vi.search(q, k=k)[1]
    assert np.array_equal(I4, ref)
    info = vi.save(tmp_path)
    assert info["flat_sq8"] is True and json.loads((tmp_path / "index_info.json").read_text())["flat_sq8"] is True
    back = VectorIndex.load(tmp_path, device=gpu)
    assert back.index_type == "FlatSQ8-GPU" and back.refine == 4 and torch.equal(back.sq_codes, vi.sq_codes)
    assert np.array_equal(back.search(q, k=k)[1], I4)
    with pytest.raises(NativeUnavailable):
        vi.search(q, k=FLAT_SQ8_MAX_K + 1)
    with pytest.raises(NativeUnavailable):
        VectorIndex(dim=D, device="cpu", index_type="flatsq8")
    with pytest.raises(NativeUnavailable):
        VectorIndex(dim=96, device=gpu, index_type="flatsq8")
