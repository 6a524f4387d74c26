"""The glue of ``CellposeRunner``: which stage runs with which parameters, whichever entry point is
taken.  ``eval`` against the network stage plus ``compute_masks``, the three layouts of a z-stack,
the parameter copies of the stack entry points (CPU, exact), the mask hand-off to the second stream
and the pipelined ``eval`` (GPU)."""
import dataclasses

import numpy as np
import pytest
import torch

from tests.test_cellpose_reference import disk_labels, flows_from_labels


@pytest.fixture(scope="module")
def cpu_runner():
    from bioengine_worker_amd.cellpose.pipeline import CellposeRunner
    from bioengine_worker_amd.models.cpnet import CPnet

    return CellposeRunner(CPnet().randomize_(0), device="cpu")


@pytest.fixture(scope="module")
def cells():
    from bioengine_worker_amd.cellpose.pipeline import synthetic_cells

    return synthetic_cells(2, 32, 32, ncells=3, seed=1)


@pytest.fixture(scope="module")
def stack():
    """One [Z, C, H, W] = 4 x 2 x 16 x 16 stack and a label volume on its grid."""
    x = np.random.default_rng(5).uniform(0, 1000, (4, 2, 16, 16)).astype(np.float32)
    m = np.zeros((4, 16, 16), np.int32)
    m[:3, 2:7, 3:9] = 1
    m[1:, 9:14, 8:15] = 2
    return x, m


# ------------------------------------------------------------------ network stage + masks == eval


@pytest.mark.unit
@pytest.mark.parametrize("diameter", [None, 15, [None, 15]], ids=["none", "scalar", "list"])
def test_eval_is_network_stage_then_compute_masks(cpu_runner, cells, diameter):
    from bioengine_worker_amd.cellpose.pipeline import EvalParams, as_batch

    r = cpu_runner
    masks, flows, styles = r.eval(cells, EvalParams(diameter=diameter))
    p = EvalParams(diameter=diameter)
    y, style, rescale = r._net_stage(as_batch(cells, r.nchan, r.device), p)
    want = r.compute_masks(y, p, rescale)
    assert torch.equal(flows, y) and torch.equal(styles, style)
    assert masks.dtype == want.dtype and torch.equal(masks, want)
    assert hasattr(masks, "diameters") == isinstance(diameter, list)
    if isinstance(diameter, list):
        assert torch.equal(masks.diameters, want.diameters) and masks.diameters.tolist() == [0.0, 15.0]
    else:
        assert rescale == (1.0 if diameter is None else r.diam_mean / 15)
    none, f2, s2 = r.eval(cells, EvalParams(diameter=diameter), compute_masks=False)
    assert none is None and torch.equal(f2, flows) and torch.equal(s2, styles)


# ------------------------------------------------------------------ stack layouts


@pytest.mark.unit
def test_stack_layouts_give_equal_results(cpu_runner, stack):
    x, m = stack
    r = cpu_runner
    layouts = {"zchw": x, "zhwc": np.ascontiguousarray(x.transpose(0, 2, 3, 1))}
    one = {"zhw": x[:, 0], "zchw": x[:, :1], "zhwc": np.ascontiguousarray(x[:, :1].transpose(0, 2, 3, 1))}
    for forms in (layouts, one):
        outs = [r.eval_stack(v, compute_masks=False, stack_batch=3) for v in forms.values()]
        tabs = [r.measure(m, v, volume=True) for v in forms.values()]
        for (none, f, s), t in zip(outs[1:], tabs[1:]):
            assert none is None and torch.equal(f, outs[0][1]) and torch.equal(s, outs[0][2])
            assert set(t) == set(tabs[0]) and t["n_cells"] == 2
            for k in ("int_mean", "int_std", "int_min", "int_max"):
                assert np.array_equal(t[k], tabs[0][k]), k
    t = r.measure(m, layouts["zhwc"], volume=True)  # both channels are there, each in its own column
    assert t["int_mean"].shape == (2, 2) and not np.array_equal(t["int_mean"][:, 0], t["int_mean"][:, 1])


@pytest.mark.unit
@pytest.mark.parametrize("shape", [(16, 16), (2, 4, 2, 16, 16)], ids=["2d", "5d"])
def test_stack_readers_reject_other_ranks(cpu_runner, shape):
    bad = np.zeros(shape, np.float32)
    with pytest.raises(ValueError, match="eval_stack expects"):
        cpu_runner.eval_stack(bad)
    with pytest.raises(ValueError, match="eval_3d expects"):
        cpu_runner.eval_3d(bad)
    with pytest.raises(ValueError, match="a z-stack is"):
        cpu_runner.measure(np.zeros((4, 16, 16), np.int32), bad, volume=True)


# ------------------------------------------------------------------ parameter copies


@pytest.mark.unit
def test_stack_entry_points_leave_the_callers_params_alone(cpu_runner, stack):
    from bioengine_worker_amd.cellpose.pipeline import EvalParams

    norm = {"percentile": [2.0, 98.0], "norm3D": False}
    p = EvalParams(normalize=norm, diameter=None, stack_batch=32)
    before = {f.name: getattr(p, f.name) for f in dataclasses.fields(p)}
    x = stack[0]
    cpu_runner.eval_stack(x, p, compute_masks=False, stack_batch=2, cellprob_threshold=1.0)
    cpu_runner.eval_3d(x, p, compute_masks=False, stack_batch=5, anisotropy=1.5)
    for f in dataclasses.fields(p):
        assert getattr(p, f.name) is before[f.name] or getattr(p, f.name) == before[f.name], f.name
    assert p.normalize is norm and norm == {"percentile": [2.0, 98.0], "norm3D": False}
    assert p.norm3d is True and p.compute_masks is True and p.stack_batch == 32 and p.anisotropy is None


# ------------------------------------------------------------------ GPU: mask hand-off, pipelined eval


@pytest.fixture(scope="module")
def gpu_runner(gpu):
    from bioengine_worker_amd.cellpose.pipeline import CellposeRunner

    return CellposeRunner(device=gpu, seed=1)


@pytest.fixture(scope="module")
def label_flows(gpu):
    ys = []
    for s in range(3):
        dP, cp = flows_from_labels(disk_labels(128, 160, 10, seed=40 + s))
        ys.append(np.concatenate([dP, cp[None]], 0))
    return torch.from_numpy(np.stack(ys)).to(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("per_image", [False, True], ids=["scalar", "per_image"])
def test_mask_hand_off_equals_compute_masks(gpu, gpu_runner, label_flows, per_image):
    """Mask recovery from fixed flows is deterministic: the masks handed off to the second stream
    are those of ``compute_masks`` on the current stream, bit for bit."""
    from bioengine_worker_amd.cellpose.pipeline import EvalParams, PerImageRescale

    r, y = gpu_runner, label_flows
    p = EvalParams(niter=0)  # niter from the rescale: 200, 100, 200 for the per-image case
    rescale = PerImageRescale([1.0, 2.0, 1.0], [None, 15.0, None]) if per_image else 1.0
    want = r.compute_masks(y, p, rescale)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(gpu))
    got = r._masks_on_side_stream(y, p, rescale, ev)
    r._mask_stream.synchronize()
    assert int(want.max()) > 0 and got.dtype == want.dtype and torch.equal(got, want)
    assert getattr(got, "label_bound", None) == getattr(want, "label_bound", None)
    assert hasattr(got, "diameters") == per_image
    if per_image:
        assert torch.equal(got.diameters, want.diameters) and got.diameters.tolist() == [0.0, 15.0, 0.0]


@pytest.mark.gpu
def test_pipelined_eval_matches_plain_eval(gpu, gpu_runner):
    """``eval`` is not bitwise repeatable on the GPU (float atomics in the style reduction), so the
    tolerances are those of ``test_cross_batch_stream_and_locked_eval_match_eval``."""
    from bioengine_worker_amd.cellpose.pipeline import synthetic_cells

    x = torch.from_numpy(synthetic_cells(4, 256, 256, ncells=25, seed=3)).to(gpu)
    mr, fr, sr = gpu_runner.eval(x, diameter=24.0)
    m, f, s = gpu_runner.eval(x, diameter=24.0, pipeline_chunks=2, pipeline_min_chunk=1)
    assert m.shape == mr.shape and f.shape == fr.shape and s.shape == sr.shape and int(mr.max()) > 0
    rel = ((f - fr).norm() / fr.norm()).item()
    diff = (m != mr).float().mean().item()
    print(f"pipelined vs plain eval: flow relative RMS {rel:.3e}, differing mask pixels {diff:.3e}")
    assert rel < 2e-3, rel
    assert diff < 1e-3, diff
