"""``be_topk_merge`` (``csrc/kernels/topk_merge.hip``) called directly on partial lists made in numpy, against
``np.lexsort((rows, -scores))[:kk]``: scores, padding and ids exact.  Integer scores in -3..3, so ties are everywhere and
the order falls to the row; rows unique per query and mapped through a permutation.  P = 600 is more ranges than the
merge workgroup has threads, so the early-stop count spans chunks."""
import numpy as np
import pytest
import torch

from bioengine_worker_amd.ops import _native

pytestmark = pytest.mark.gpu

Q = 3


def _candidates(case, P, kk, rng):
    """-> (scores, rows, range) of one query's candidates; a range keeps its first kk under the order."""
    n = {"random": 3 * kk + 2 * P, "last": 2 * kk + P if P > 1 else 0, "one_full": 2 * kk, "few": kk // 2,
         "zeros": 3 * kk + 2 * P}[case]
    sc = rng.integers(-3, 4, n).astype(np.float32)
    at = rng.integers(0, P, n)
    if case == "last":  # the best kk all in the last range, every other range holds lower scores
        sc, at = np.minimum(sc, 2), rng.integers(0, max(P - 1, 1), n)
        sc, at = np.concatenate([sc, np.full(kk, 3, np.float32)]), np.concatenate([at, np.full(kk, P - 1)])
    if case == "one_full":  # one range full, all others pure padding
        at[:] = P // 2
    if case == "zeros":  # +0.0 and -0.0 count as equal
        sc = rng.choice(np.array([-1.0, -0.0, 0.0, 1.0], np.float32), n)
    return sc, rng.permutation(2 * len(sc) + 8)[:len(sc)].astype(np.int32), at


def _partials(sc, rows, at, P, kk):
    """The ranges' lists [P, kk], each ordered and cut to kk, padded with (-inf, -1)."""
    ps, pr = np.full((P, kk), -np.inf, np.float32), np.full((P, kk), -1, np.int32)
    o = np.lexsort((rows, -sc, at))
    a = at[o]
    rank = np.arange(len(o)) - np.searchsorted(a, a)
    keep = rank < kk
    ps[a[keep], rank[keep]], pr[a[keep], rank[keep]] = sc[o][keep], rows[o][keep]
    return ps, pr


@pytest.mark.parametrize("case", ["random", "last", "one_full", "few", "zeros"])
@pytest.mark.parametrize("kk", [1, 20, 1024])
@pytest.mark.parametrize("P", [1, 2, 17, 600])
def test_topk_merge_exact(gpu, P, kk, case):
    rng = np.random.default_rng(1000 * P + kk)
    ids = rng.permutation(2 * (3 * kk + 2 * P) + 8).astype(np.int64)
    part_s, part_r = np.empty((Q, P, kk), np.float32), np.empty((Q, P, kk), np.int32)
    S, I = np.full((Q, kk), -np.inf, np.float32), np.full((Q, kk), -1, np.int64)
    for qi in range(Q):
        part_s[qi], part_r[qi] = _partials(*_candidates(case, P, kk, rng), P, kk)
        has = part_r[qi] >= 0
        sc, rows = part_s[qi][has], part_r[qi][has]
        o = np.lexsort((rows, -sc))[:kk]
        S[qi, :len(o)], I[qi, :len(o)] = sc[o] + 0.0, ids[rows[o]]  # + 0.0: a zero comes out as +0.0
    assert (I == -1).any() == (case == "few")  # only that case pads its result
    ps, pr, di = (torch.from_numpy(a).to(gpu) for a in (part_s, part_r, ids))
    got = []
    for _ in range(2):
        out_s = torch.empty(Q, kk, dtype=torch.float32, device=gpu)
        out_i = torch.empty(Q, kk, dtype=torch.int64, device=gpu)
        with torch.cuda.device(gpu):
            _native.call("be_topk_merge", _native.ptr(ps), _native.ptr(pr), _native.ptr(di), Q, P, kk, _native.ptr(out_s),
                         _native.ptr(out_i), _native.stream(gpu))
        got.append((out_s.cpu().numpy(), out_i.cpu().numpy()))
    assert np.array_equal(got[0][0].view(np.uint32), S.view(np.uint32)) and np.array_equal(got[0][1], I)
    assert np.array_equal(got[0][0].view(np.uint32), got[1][0].view(np.uint32)) and np.array_equal(got[0][1], got[1][1])
