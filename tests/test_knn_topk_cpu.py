"""The host side of the fused neighbour tables (``search/umap.py``) that needs no GPU."""
import numpy as np
import pytest
import torch

from bioengine_worker_amd.ops import _native
from bioengine_worker_amd.search import umap as gu


@pytest.mark.parametrize("d", [8, 32, 768])
def test_split_bf16_k3(d):
    """``[hi, hi, lo] . [hi', lo', hi']`` drops ``lo.lo'`` and the residuals of the second rounding: 3 * 2^-18 on
    unit rows, so 2^-15 holds with room."""
    x = torch.from_numpy(np.random.default_rng(d).standard_normal((40, d))).float()
    x = x / x.norm(dim=1, keepdim=True)
    A, B = gu.split_bf16_k3(x), gu.split_bf16_k3(x[:7], right=True)
    K = A.shape[1]
    assert A.dtype == B.dtype == torch.bfloat16 and B.shape == (7, K) and K % 32 == 0 and 3 * d <= K < 3 * d + 32
    assert not A[:, 3 * d:].any() and not B[:, 3 * d:].any()
    err = (A.double() @ B.double().T - x.double() @ x[:7].double().T).abs().max().item()
    print(f"d={d}: K'={K}, largest split error {err:.3e}")
    assert err <= 2.0 ** -15


def test_methods_on_cpu_tensor():
    x = torch.from_numpy(np.random.default_rng(1).standard_normal((90, 8))).float()
    with pytest.raises(_native.NativeUnavailable):
        gu.knn_table_gpu(x, 5, method="fused")
    with pytest.raises(_native.NativeUnavailable):
        gu.knn_query_table_gpu(x[:9], x, 5, method="fused")
    for auto, plain in ((gu.knn_table_gpu(x, 5, method="auto"), gu.knn_table_gpu(x, 5, method="torch")),
                        (gu.knn_query_table_gpu(x[:9], x, 5), gu.knn_query_table_gpu(x[:9], x, 5, method="torch"))):
        assert auto[0].knn_method == "torch" and torch.equal(auto[0], plain[0]) and torch.equal(auto[1], plain[1])
