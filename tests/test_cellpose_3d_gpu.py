"""Cellpose do_3D on the GPU (``csrc/kernels/cellpose_dynamics3d.hip``): the view accumulator must equal
``reference.combine_views3d`` bit for bit; on capped flows (end points mid-bin, see
``cellpose3d_cases``) the dynamics, the histogram and the final masks equal the oracle exactly; on unit
flows they match it as closely as the 2-D test asks (same count, match fraction > 0.99);
``get_masks3d_gpu`` equals the oracle on every hand-built rule case; ``CellposeRunner.eval_3d`` equals
its pieces composed by hand."""
import numpy as np
import pytest
import torch

import cellpose3d_cases as cc
from bioengine_worker_amd.cellpose import reference as ref

pytestmark = pytest.mark.gpu


def _field(v, gpu):
    return torch.from_numpy(np.concatenate([v["dP"], v["cellprob"][None]])).to(gpu)


# ------------------------------------------------------------------ views


@pytest.mark.parametrize("Z,H,W,chunk", [(19, 33, 45, 32), (5, 7, 33, 33), (3, 70, 37, 1), (2, 2, 2, 7)])
def test_accum_views_equal_oracle(gpu, Z, H, W, chunk):
    """ZY chunks of 33 planes (a full transpose tile and a ragged one-plane rest), of 1 plane, and
    y extents that are no multiple of the 32-wide tile."""
    from bioengine_worker_amd.cellpose.gpu import combine_views3d_gpu

    rng = np.random.default_rng(Z * 1000 + W)
    yx = rng.standard_normal((Z, 3, H, W)).astype(np.float32)
    zx = rng.standard_normal((H, 3, Z, W)).astype(np.float32)
    zy = rng.standard_normal((W, 3, Z, H)).astype(np.float32)
    dP, cp = ref.combine_views3d(yx, zx, zy)
    acc = combine_views3d_gpu(*(torch.from_numpy(a).to(gpu) for a in (yx, zx, zy)), chunk=chunk)
    assert acc.shape == (4, Z, H, W) and acc.dtype == torch.float32
    assert torch.equal(acc[:3].cpu(), torch.from_numpy(dP)) and torch.equal(acc[3].cpu(), torch.from_numpy(cp))


def test_accum_view_rejects_misfits(gpu):
    from bioengine_worker_amd.cellpose.gpu import accum_view3d

    acc = torch.zeros(4, 3, 5, 7, device=gpu)
    with pytest.raises(ValueError, match="does not fit"):
        accum_view3d(acc, torch.zeros(2, 3, 5, 7, device=gpu), 0, 2)  # planes 2, 3 of 3
    with pytest.raises(ValueError, match="does not fit"):
        accum_view3d(acc, torch.zeros(2, 3, 5, 7, device=gpu), 1, 0)  # a YX chunk handed in as ZX


# ------------------------------------------------------------------ dynamics


@pytest.mark.parametrize("name", ["a", "b", "c", "edge"])
def test_capped_flows_exact(gpu, name):
    from bioengine_worker_amd.cellpose.gpu import compute_masks3d_gpu, follow_flows3d_gpu

    v, o = cc.volume(name, "capped"), cc.oracle(name, "capped")
    want_hist, want_pos = cc.hist_pos(o["bins"], o["inds"], v["shape"])
    flow = _field(v, gpu)
    hist, pos = follow_flows3d_gpu(flow)
    assert pos.dtype == torch.int32 and hist.dtype == torch.int32
    assert torch.equal(pos.cpu(), torch.from_numpy(want_pos))  # every foreground voxel's bin, -1 elsewhere
    assert torch.equal(hist.cpu(), torch.from_numpy(want_hist))
    m = compute_masks3d_gpu(flow[:3], flow[3])
    assert m.dtype == torch.int32 and m.shape == v["shape"] and m.device.type == "cuda"
    assert torch.equal(m.cpu(), torch.tensor(o["masks"]))
    assert int(m.max()) == v["n"]


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_unit_flows_match(gpu, name):
    from bioengine_worker_amd.cellpose.gpu import compute_masks3d_gpu

    v, o = cc.volume(name, "unit"), cc.oracle(name, "unit")
    m = compute_masks3d_gpu(_field(v, gpu)).cpu().numpy()
    frac = cc.match_fraction(m, o["masks"])
    print(f"unit {name}: instances {int(m.max())} (oracle {int(o['masks'].max())}), match fraction {frac:.5f}")
    assert int(m.max()) == int(o["masks"].max()) == v["n"]
    assert frac > 0.99


def test_launch_variants_identical(gpu):
    from bioengine_worker_amd.cellpose.gpu import follow_flows3d_gpu

    for name, kind in (("a", "unit"), ("edge", "capped")):
        flow = _field(cc.volume(name, kind), gpu)
        h0, p0 = follow_flows3d_gpu(flow, variant=0)
        h1, p1 = follow_flows3d_gpu(flow, variant=1)
        assert torch.equal(p0, p1) and torch.equal(h0, h1) and int(h0.sum()) == int((p0 >= 0).sum()) > 0


def test_cellprob_threshold_and_niter(gpu):
    from bioengine_worker_amd.cellpose.gpu import follow_flows3d_gpu

    v = cc.volume("b", "capped")
    flow = _field(v, gpu)
    hist, pos = follow_flows3d_gpu(flow, niter=0)  # no step: every foreground voxel bins itself
    z, y, x = np.nonzero(v["truth"])
    Hp, Wp = v["shape"][1] + 40, v["shape"][2] + 40
    want = np.full(v["shape"], -1, np.int32)
    want[z, y, x] = ((z + 20) * Hp + (y + 20)) * Wp + (x + 20)
    assert torch.equal(pos.cpu(), torch.from_numpy(want)) and int(hist.max()) == 1
    hist, pos = follow_flows3d_gpu(flow, cellprob_threshold=5.0)  # cellprob is +-5: nothing is above 5
    assert int(hist.sum()) == 0 and bool((pos == -1).all())


def test_tiny_and_empty_volumes(gpu):
    from bioengine_worker_amd.cellpose.gpu import compute_masks3d_gpu, follow_flows3d_gpu

    v, o = cc.volume("flat", "capped"), cc.oracle("flat", "capped")  # [1, 5, 7]: an axis of length 1
    want_hist, want_pos = cc.hist_pos(o["bins"], o["inds"], v["shape"])
    flow = _field(v, gpu)
    hist, pos = follow_flows3d_gpu(flow)
    assert torch.equal(pos.cpu(), torch.from_numpy(want_pos)) and torch.equal(hist.cpu(), torch.from_numpy(want_hist))
    m = compute_masks3d_gpu(flow, max_size_fraction=1.0)
    assert torch.equal(m.cpu(), torch.tensor(o["masks"])) and int(m.sum()) == 35
    # no foreground at all
    z = compute_masks3d_gpu(torch.zeros(3, 5, 7, 9, device=gpu), -torch.ones(5, 7, 9, device=gpu))
    assert z.shape == (5, 7, 9) and z.dtype == torch.int32 and not bool(z.any())
    with pytest.raises(ValueError, match="too large"):
        compute_masks3d_gpu(torch.zeros(4, 0, 50000, 50000, device=gpu))


# ------------------------------------------------------------------ seeds / expansion / fill


def _check_get_masks(gpu, shape, p, inds, **kw):
    from bioengine_worker_amd.cellpose.gpu import get_masks3d_gpu

    want = ref.get_masks3d(p, inds, shape, **kw)
    hist, pos = cc.hist_pos(ref.end_bins3d(p, shape), inds, shape)
    got = get_masks3d_gpu(torch.from_numpy(hist).to(gpu), torch.from_numpy(pos).to(gpu), shape, **kw)
    assert got.dtype == torch.int32 and tuple(got.shape) == tuple(shape)
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    return want


@pytest.mark.parametrize("name", sorted(cc.RULES))
def test_get_masks_rules(gpu, name):
    shape, (p, inds) = cc.RULES[name]()
    want = _check_get_masks(gpu, shape, p, inds)
    assert want.any()
    if name == "oversize":
        assert (_check_get_masks(gpu, shape, p, inds, max_size_fraction=0.7) > 0).sum() == 219


def test_get_masks_lattice_of_seeds(gpu):
    """729 seeds of equal count: more than one workgroup expands (four per workgroup), ordered by
    the raster tie-break alone."""
    shape, (p, inds) = cc.lattice()
    assert int(_check_get_masks(gpu, shape, p, inds).max()) == 729


def test_get_masks_window_at_the_histogram_border(gpu):
    """Seeds in the first and last bins an end point can have: their windows end 15 bins inside the
    padded volume; a hand-made histogram may also put one in the very corner, where the window is cut."""
    from bioengine_worker_amd.cellpose.gpu import get_masks3d_gpu

    shape = (9, 13, 29)
    _check_get_masks(gpu, shape, *cc._points(shape, [((0, 0, 0), 12), ((0, 0, 1), 4), ((8, 12, 28), 12), ((8, 12, 27), 3)]))
    hist = torch.zeros(49, 53, 69, dtype=torch.int32)
    hist[0, 0, 0], hist[0, 0, 1], hist[48, 52, 68], hist[47, 51, 67] = 12, 3, 20, 3
    pos = torch.full(shape, -1, dtype=torch.int32)
    pos.view(-1)[:4] = torch.tensor([0, 1, 49 * 53 * 69 - 1, (47 * 53 + 51) * 69 + 67], dtype=torch.int32)
    got = get_masks3d_gpu(hist.to(gpu), pos.to(gpu), shape).cpu()
    assert got.view(-1)[:4].tolist() == [1, 1, 2, 2] and int((got > 0).sum()) == 4


@pytest.mark.parametrize("min_size", [0, 15])
def test_fill_holes3d(gpu, min_size):
    from bioengine_worker_amd.cellpose.gpu import fill_holes3d_gpu

    m = np.zeros((8, 21, 23), np.int32)
    m[1:4, 2:9, 2:9] = 3
    m[2, 4:6, 4:6] = 0  # in-plane hole
    m[1, 3, 3] = 0
    m[:, 11:20, 11:20] = 7  # a ring through every plane with another instance inside its hole
    m[:, 13:18, 13:18] = 0
    m[4, 14:17, 14:17] = 2
    m[0:2, 2:5, 15:17] = 5  # 12 voxels: below min_size 15
    m[5:8, 2:9, 2:9] = 9
    m[6, 2:9, 5] = 0  # a channel open in its own plane: stays
    m[:, 0:2, 20:22] = 11  # 4 voxels per plane, 32 in all: kept
    want = ref.fill_holes_and_remove_small_masks3d(m, min_size)
    got = fill_holes3d_gpu(torch.from_numpy(m).to(gpu), min_size)
    assert got.dtype == torch.int32 and torch.equal(got.cpu(), torch.from_numpy(want))
    assert int(want.max()) == (6 if min_size == 0 else 4)
    got = fill_holes3d_gpu(torch.from_numpy(m).to(gpu), min_size, nlab=40)  # a loose label bound
    assert torch.equal(got.cpu(), torch.from_numpy(want))


# ------------------------------------------------------------------ runner


def test_eval_3d_end_to_end(gpu):
    import dataclasses

    from bioengine_worker_amd.cellpose import gpu as cg
    from bioengine_worker_amd.cellpose.pipeline import CellposeRunner, EvalParams, as_batch, synthetic_cells

    runner = CellposeRunner(device=gpu)
    stack = synthetic_cells(16, 64, 80, ncells=12, seed=2)  # [16, 2, 64, 80]
    masks, flows, styles = runner.eval_3d(stack, stack_batch=24)
    Z, H, W = 16, 64, 80
    assert masks.shape == (Z, H, W) and masks.dtype == torch.int32 and masks.device.type == "cuda"
    assert flows.shape == (4, Z, H, W) and flows.dtype == torch.float32 and bool(torch.isfinite(flows).all())
    assert styles.dim() == 1 and bool(torch.isfinite(styles).all())
    # the pieces by hand: stack-normalised volume, three whole views, combine, 3-D masks
    x = as_batch(stack, runner.nchan, gpu)
    C = x.shape[1]
    xn = cg.normalize99(x.permute(1, 0, 2, 3).reshape(1, C, Z * H, W)).reshape(C, Z, H, W).permute(1, 0, 2, 3).contiguous()
    p = EvalParams(normalize=False)
    ys = []
    for perm in ((0, 1, 2, 3), (2, 1, 0, 3), (3, 1, 0, 2)):
        xv = xn.permute(*perm).contiguous()
        ys.append(torch.cat([runner._net_stage(xv[i: i + 24], dataclasses.replace(p))[0] for i in range(0, xv.shape[0], 24)]))
    acc = cg.combine_views3d_gpu(*ys)
    assert torch.equal(flows, acc)
    dP, cp = ref.combine_views3d(*(y.cpu().numpy() for y in ys))  # the accumulator is the oracle's sum, bit for bit
    assert torch.equal(acc[:3].cpu(), torch.from_numpy(dP)) and torch.equal(acc[3].cpu(), torch.from_numpy(cp))
    assert torch.equal(masks, cg.compute_masks3d_gpu(acc[:3], acc[3]))
    # anisotropy: masks at the input depth, flows at the resampled one
    m2, f2, _ = runner.eval_3d(stack, stack_batch=24, anisotropy=1.5)
    assert m2.shape == (Z, H, W) and f2.shape == (4, 24, H, W) and bool(torch.isfinite(f2).all())


def test_eval_3d_smallest_depth(gpu):
    """MIN_DEPTH_3D planes: the ZX and ZY views are two rows high (padded to the network's 32-row tile)."""
    from bioengine_worker_amd.cellpose.pipeline import CellposeRunner, synthetic_cells

    runner = CellposeRunner(device=gpu)
    Z = CellposeRunner.MIN_DEPTH_3D
    stack = synthetic_cells(Z, 40, 48, ncells=6, seed=3)
    m, f, s = runner.eval_3d(stack)
    assert m.shape == (Z, 40, 48) and f.shape == (4, Z, 40, 48) and bool(torch.isfinite(f).all()) and s.dim() == 1
    with pytest.raises(ValueError, match="at least"):
        runner.eval_3d(stack[:1])
