"""z-stack stitching on the GPU: ``stitch3d_gpu`` (``csrc/kernels/cellpose_stitch.hip``) must equal the
numpy oracle ``reference.stitch3d`` exactly on every input, whatever the arrival order of its
atomics, the hash capacity or the label bound; ``CellposeRunner.eval_stack`` end to end."""
import numpy as np
import pytest
import torch

import stitch_cases as sc
from bioengine_worker_amd.cellpose import reference as ref

pytestmark = pytest.mark.gpu


def _check(gpu, masks, t=0.25, min_size=0, **kw):
    from bioengine_worker_amd.cellpose.gpu import stitch3d_gpu

    want = torch.from_numpy(ref.stitch3d(masks, t, min_size))
    M = torch.from_numpy(np.ascontiguousarray(masks)).to(gpu)
    got = stitch3d_gpu(M, t, min_size, **kw)
    assert got.shape == M.shape and got.dtype == torch.int32 and got.device == M.device
    assert torch.equal(got.cpu(), want)
    return want


def test_prisms(gpu):
    truth, masks = sc.prisms()
    assert int(_check(gpu, masks).max()) == int(truth.max())


@pytest.fixture(scope="module")
def sphere_masks():
    return sc.spheres()[1]


@pytest.mark.parametrize("t,min_size,K", [(0.25, 0, 15), (0.25, 60, 10), (0.1, 0, 10)])
def test_spheres(gpu, sphere_masks, t, min_size, K):
    assert int(_check(gpu, sphere_masks, t, min_size).max()) == K


@pytest.mark.parametrize("name", sorted(sc.EDGE_CASES))
def test_rules_and_edges(gpu, name):
    m = sc.EDGE_CASES[name]()
    _check(gpu, m, 0.25)
    _check(gpu, m, 0.26)  # the threshold pair (IoU exactly 0.25) no longer links
    _check(gpu, m, 0.25, min_size=30)


@pytest.mark.parametrize("H,W", [(37, 53), (1, 7)])
def test_ragged_sizes(gpu, H, W):
    """H * W no multiple of 4: misaligned planes in the overlap pass, a vector straddling two planes
    and the scalar tail in the relabel pass."""
    m = sc.ragged(H, W)
    assert m.any()
    _check(gpu, m, 0.25)
    _check(gpu, m, 0.05, min_size=2)


@pytest.fixture(scope="module")
def many():
    m = sc.many_labels()
    assert m.shape == (5, 200, 200) and int(m.max()) == 1600
    return m


def test_many_labels(gpu, many):
    """1,600 labels per plane: more than one workgroup's labels in the numbering walk, more pairs per
    workgroup than its LDS table holds, several workgroups adding to one key."""
    want = _check(gpu, many, 0.25)
    assert int(want.max()) == 1600  # IoU 6/12 links every square through the stack
    _check(gpu, many, 0.51)  # nothing links: 8,000 instances
    _check(gpu, many, 0.25, min_size=46)  # 45 voxels each: all dropped


def test_contention_one_key(gpu):
    _check(gpu, sc.one_large(), 0.25)


def test_forced_overflow_retries(gpu, many):
    """64 slots for ~3,200 pairs: the launch must return with the overflow word set (bounded probing,
    no spinning on a full table) and the doubled-capacity retries give the identical result."""
    _check(gpu, many, 0.25, capacity=64)


def test_nlab_bound(gpu, many, sphere_masks):
    _check(gpu, many, 0.25, nlab=1601)
    _check(gpu, many, 0.25, nlab=5000)
    _check(gpu, sphere_masks, 0.25, nlab=64)


def test_non_contiguous_and_offset_views(gpu, sphere_masks):
    """A slice of a larger stack starts at an address that is no multiple of 16 bytes."""
    from bioengine_worker_amd.cellpose.gpu import stitch3d_gpu

    big = torch.zeros(6 * 37 * 53 + 1, dtype=torch.int32, device=gpu)
    m = sc.ragged(37, 53, Z=6)
    view = big[1:].view(6, 37, 53)
    view.copy_(torch.from_numpy(m))
    assert view.data_ptr() % 16 == 4
    assert torch.equal(stitch3d_gpu(view, 0.25).cpu(), torch.from_numpy(ref.stitch3d(m, 0.25)))


def test_eval_stack_end_to_end(gpu):
    from bioengine_worker_amd.cellpose.gpu import normalize99
    from bioengine_worker_amd.cellpose.pipeline import CellposeRunner, as_batch, synthetic_cells

    runner = CellposeRunner(device=gpu)
    stack = synthetic_cells(4, 128, 128, ncells=12, seed=2)
    prm = {"flow_threshold": 0.0}  # a random network's flows fail the QC, which would leave nothing to stitch
    masks, flows, styles = runner.eval_stack(stack, stitch_threshold=0.25, **prm)
    assert masks.shape == (4, 128, 128) and masks.dtype == torch.int32 and masks.device.type == "cuda"
    assert flows.shape == (4, 3, 128, 128) and styles.shape[0] == 4
    # the same runner's eval on the stack-normalised planes, compared on the same device
    x = as_batch(stack, runner.nchan, gpu)
    Z, C, H, W = x.shape
    xn = normalize99(x.permute(1, 0, 2, 3).reshape(1, C, Z * H, W)).reshape(C, Z, H, W).permute(1, 0, 2, 3).contiguous()
    pm, py, _ = runner.eval(xn, normalize=False, **prm)
    assert int(pm.max()) > 0
    want = ref.stitch3d(pm.cpu().numpy(), 0.25, min_size=15)
    assert torch.equal(masks.cpu(), torch.from_numpy(want))
    assert torch.equal(flows, py)
    m0, _, _ = runner.eval_stack(stack, stitch_threshold=0.0, **prm)
    assert torch.equal(m0, pm)
