"""Cellpose do_3D, CPU: the numpy / torch-CPU oracle in ``cellpose.reference`` (``combine_views3d``,
``follow_flows3d``, ``get_masks3d``, ``fill_holes_and_remove_small_masks3d``, ``compute_masks3d`` -- the
yardstick of the HIP kernels in ``test_cellpose_3d_gpu.py``), ``CellposeRunner.eval_3d`` on a CPU runner
and the ``do_3D`` mode of the Cellpose app's ``infer``."""
import asyncio
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

import cellpose3d_cases as cc
from bioengine_worker_amd.cellpose import reference as ref

ROOT = Path(__file__).resolve().parents[1]
APP_MAIN = ROOT / "apps" / "cellpose-finetuning" / "main.py"


# ------------------------------------------------------------------ views


def _coded_views(Z, H, W):
    """View arrays whose values encode (view, channel, z, y, x) of the voxel they belong to."""
    z, y, x = np.meshgrid(np.arange(Z), np.arange(H), np.arange(W), indexing="ij")
    vox = (z * 10 + y) * 10 + x  # every code, and every sum of three of them, is below 2^24: exact in fp32

    def code(view, ch):
        return (vox + (view * 3 + ch + 1) * 100000).astype(np.float32)  # [Z, H, W]

    yx = np.stack([code(0, c) for c in range(3)], 1)  # [Z, 3, H, W]
    zx = np.stack([code(1, c).transpose(1, 0, 2) for c in range(3)], 1)  # [H, 3, Z, W]
    zy = np.stack([code(2, c).transpose(2, 0, 1) for c in range(3)], 1)  # [W, 3, Z, H]
    return vox, yx, zx, zy


@pytest.mark.unit
def test_combine_views3d_routes_every_channel():
    Z, H, W = 3, 5, 7
    vox, yx, zx, zy = _coded_views(Z, H, W)
    assert yx.shape == (Z, 3, H, W) and zx.shape == (H, 3, Z, W) and zy.shape == (W, 3, Z, H)
    dP, cp = ref.combine_views3d(yx, zx, zy)
    assert dP.shape == (3, Z, H, W) and cp.shape == (Z, H, W) and dP.dtype == cp.dtype == np.float32
    M = 100000
    # view v, channel c carries (3 v + c + 1) M + voxel code
    assert np.array_equal(dP[0], 2 * vox + (4 + 7) * M)  # dZ = zx[0] + zy[0]
    assert np.array_equal(dP[1], 2 * vox + (1 + 8) * M)  # dY = yx[0] + zy[1]
    assert np.array_equal(dP[2], 2 * vox + (2 + 5) * M)  # dX = yx[1] + zx[1]
    assert np.array_equal(cp, 3 * vox + (3 + 6 + 9) * M)  # cellprob = yx[2] + zx[2] + zy[2]


@pytest.mark.unit
def test_combine_views3d_addition_order():
    """(yx + zx) + zy, not any other association: 1 + 2^-24 + 2^-24 rounds differently."""
    one = np.ones((2, 3, 2, 2), np.float32)
    tiny = np.full((2, 3, 2, 2), 2.0 ** -24, np.float32)
    _, cp = ref.combine_views3d(tiny, tiny, one)
    assert (cp == np.float32(1.0) + np.float32(2.0 ** -23)).all()
    _, cp = ref.combine_views3d(one, tiny, tiny)
    assert (cp == 1.0).all()


# ------------------------------------------------------------------ oracle round trip


@pytest.mark.unit
@pytest.mark.parametrize("name,kind", [("a", "capped"), ("a", "unit"), ("b", "capped"), ("b", "unit"), ("c", "capped"),
                                       ("c", "unit"), ("edge", "capped"), ("flat", "capped")])
def test_oracle_recovers_ellipsoids(name, kind):
    v, o = cc.volume(name, kind), cc.oracle(name, kind)
    found, worst = cc.match(o["masks"], v["truth"])
    assert found == v["n"]
    assert worst > 0.9
    assert not o["masks"][v["truth"] == 0].any()
    m = ref.compute_masks3d(v["dP"], v["cellprob"], max_size_fraction=1.0 if name == "flat" else 0.4)
    assert m.dtype == np.int32 and np.array_equal(m, o["masks"])


@pytest.mark.unit
def test_follow_flows3d_fixed_point_and_degenerate_axes():
    v, o = cc.volume("b", "capped"), cc.oracle("b", "capped")
    shape, specs = cc.VOLUMES["b"]
    lab = v["truth"][o["inds"]]
    for i, s in enumerate(specs):
        want = np.array(s[:3], np.float32) + 0.5  # p* = (c + 0.5) (L - 1) / L = k + 0.5
        assert np.abs(o["p"][:, lab == i + 1] - want[:, None]).max() < 0.25
    # an axis of length 1 keeps its position and samples its only plane with weight 1
    dP = np.zeros((3, 1, 5, 7), np.float32)
    dP[2] = 5.0  # one voxel per step along +x
    p, inds = ref.follow_flows3d(dP, np.ones((1, 5, 7), np.float32), 0.0, 1)
    assert np.isfinite(p).all() and (p[0] == 0).all() and np.array_equal(p[1], inds[1].astype(np.float32))
    # voxel (0, 2, 3) samples y = 2 * 5 / 4 - 0.5 = 2 and x = 3 * 7 / 6 - 0.5 = 3 exactly: a whole step
    k = int(np.nonzero((inds[1] == 2) & (inds[2] == 3))[0][0])
    assert np.abs(p[:, k] - np.array([0.0, 2.0, 4.0])).max() < 1e-5
    p, inds = ref.follow_flows3d(dP, np.ones((1, 5, 7), np.float32), 0.0, 12)
    assert (p[2] <= 6.0).all() and (p[2] > 5.5).all() and (p[2] == 6.0).any()  # clamped to L - 1
    p, inds = ref.follow_flows3d(dP, -np.ones((1, 5, 7), np.float32), 0.0, 3)
    assert p.shape == (3, 0)


# ------------------------------------------------------------------ get_masks3d rules


def _labels_at(shape, p, inds, bins):
    """Label of the voxels whose end point is in ``bins`` [(z, y, x), ...] (-1: several labels)."""
    m = ref.get_masks3d(p, inds, shape)
    pt = p.astype(np.int64)
    out = []
    for b in bins:
        sel = (pt[0] == b[0]) & (pt[1] == b[1]) & (pt[2] == b[2])
        labs = np.unique(m[inds][sel])
        out.append(int(labs[0]) if len(labs) == 1 else -1)
    return m, out


@pytest.mark.unit
def test_rule_count_and_support_thresholds():
    shape, (p, inds) = cc.rule_count_10_vs_11()
    m, labs = _labels_at(shape, p, inds, [(4, 6, 5), (4, 6, 19)])
    assert labs == [0, 1] and int(m.max()) == 1  # 10 points: no seed; 11: a seed
    shape, (p, inds) = cc.rule_support_2_vs_3()
    m, labs = _labels_at(shape, p, inds, [(4, 6, 10), (4, 6, 9), (4, 6, 11)])
    assert labs == [1, 0, 1]  # 2 points: outside the support; 3: inside


@pytest.mark.unit
def test_rule_ties_and_overlaps():
    shape, (p, inds) = cc.rule_equal_maxima()
    m, labs = _labels_at(shape, p, inds, [(4, 5, 10), (4, 6, 12), (4, 5, 7), (4, 5, 6), (4, 5, 5)])
    # both seed; the raster-later one (expanded last) owns everything it reaches, the other seed's bin included
    assert int(m.max()) == 2 and labs == [2, 2, 2, 1, 1]
    shape, (p, inds) = cc.rule_unequal_overlap()
    m, labs = _labels_at(shape, p, inds, [(4, 6, 8), (4, 6, 10), (4, 6, 12), (4, 6, 13), (4, 6, 14), (4, 6, 17)])
    # the seed of 20 is raster-earlier but larger: expanded last, it wins the bridge and both seed bins
    assert int(m.max()) == 2 and labs == [2, 2, 2, 2, 1, 1]


@pytest.mark.unit
def test_rule_dilation_connectivity_and_reach():
    shape, (p, inds) = cc.rule_gap()
    _, labs = _labels_at(shape, p, inds, [(4, 6, 10), (4, 6, 12), (4, 6, 13)])
    assert labs == [1, 0, 0]  # a one-bin gap is not crossed
    shape, (p, inds) = cc.rule_diagonal()
    _, labs = _labels_at(shape, p, inds, [(4, 6, 10), (5, 7, 11), (6, 8, 12), (6, 8, 13)])
    assert labs == [1, 1, 1, 1]  # a corner contact (26-connectivity) is crossed
    shape, (p, inds) = cc.rule_far_reach()
    _, labs = _labels_at(shape, p, inds, [(4, 6, 5 + d) for d in range(8)])
    assert labs == [1, 1, 1, 1, 1, 1, 0, 0]  # five dilations: five bins from the seed


@pytest.mark.unit
def test_rule_oversize_and_empty():
    shape, (p, inds) = cc.rule_oversize()
    m = ref.get_masks3d(p, inds, shape)
    assert int(m.max()) == 1 and (m > 0).sum() == 30  # the 189-voxel object (60 %) is dropped
    assert (ref.get_masks3d(p, inds, shape, max_size_fraction=0.7) > 0).sum() == 219
    empty = ref.get_masks3d(np.zeros((3, 0), np.float32), tuple(np.zeros(0, np.int64) for _ in range(3)), (5, 7, 9))
    assert empty.shape == (5, 7, 9) and empty.dtype == np.int32 and not empty.any()
    assert not ref.compute_masks3d(np.zeros((3, 5, 7, 9), np.float32), -np.ones((5, 7, 9), np.float32)).any()


@pytest.mark.unit
def test_lattice_every_bin_is_a_seed():
    shape, (p, inds) = cc.lattice()
    m = ref.get_masks3d(p, inds, shape)
    assert int(m.max()) == 729 and (np.bincount(m.ravel())[1:] == 11).all()
    assert np.array_equal(m[inds][::11], np.arange(1, 730))  # equal counts: raster order


# ------------------------------------------------------------------ fill / min_size


@pytest.mark.unit
def test_fill_in_plane_hole_and_3d_cavity():
    m = np.zeros((5, 9, 9), np.int32)
    m[1:4, 2:7, 2:7] = 3
    m[2, 4, 4] = 0  # a cavity closed in 3-D and in its own plane: filled
    m[1, 3, 3] = 0  # a pit in the bottom face: a hole of plane 1, filled plane by plane
    out = ref.fill_holes_and_remove_small_masks3d(m, 0)
    assert out.dtype == np.int32 and (out[1:4, 2:7, 2:7] == 1).all() and (out > 0).sum() == 75
    # a tube along y: closed by planes above and below in z, but open in every z-plane -> stays open
    t = np.zeros((5, 9, 9), np.int32)
    t[1:4, 1:8, 2:7] = 1
    t[2, 1:8, 4] = 0  # channel through the whole box along y: touches the box border in plane 2
    out = ref.fill_holes_and_remove_small_masks3d(t, 0)
    assert (out[2, 1:8, 4] == 0).all() and np.array_equal(out, t)
    # a cavity open only along z is closed in every plane it crosses: filled, although open in 3-D
    c = np.zeros((5, 9, 9), np.int32)
    c[0:5, 2:7, 2:7] = 1
    c[:, 4, 4] = 0
    out = ref.fill_holes_and_remove_small_masks3d(c, 0)
    assert (out[:, 2:7, 2:7] == 1).all()


@pytest.mark.unit
def test_fill_claims_only_background():
    m = np.zeros((3, 11, 11), np.int32)
    m[:, 1:10, 1:10] = 1
    m[:, 3:8, 3:8] = 0
    m[1, 4:7, 4:7] = 2  # another instance inside the ring's hole: not overwritten
    out = ref.fill_holes_and_remove_small_masks3d(m, 0)
    assert (out[1, 4:7, 4:7] == 2).all() and (out[1, 3, 3:8] == 1).all() and (out[0, 3:8, 3:8] == 1).all()


@pytest.mark.unit
def test_min_size_counts_the_whole_instance():
    m = np.zeros((8, 9, 9), np.int32)
    m[:, 1:3, 1:3] = 2  # 4 voxels per plane, 32 in all: kept at min_size 15
    m[0:2, 5:8, 5:7] = 5  # 12 voxels: dropped
    m[4, 5, 5] = 9
    out = ref.fill_holes_and_remove_small_masks3d(m, 15)
    assert set(np.unique(out)) == {0, 1} and np.array_equal(out > 0, m == 2)
    out = ref.fill_holes_and_remove_small_masks3d(m, 0)
    assert set(np.unique(out)) == {0, 1, 2, 3}  # ids 1..K in id order
    assert (out[m == 2] == 1).all() and (out[m == 5] == 2).all() and (out[m == 9] == 3).all()


# ------------------------------------------------------------------ wrappers on CPU tensors


@pytest.mark.unit
def test_cpu_tensors_run_the_oracle():
    from bioengine_worker_amd.cellpose import gpu

    v, o = cc.volume("b", "capped"), cc.oracle("b", "capped")
    dP, cp = torch.from_numpy(v["dP"].copy()), torch.from_numpy(v["cellprob"].copy())
    m = gpu.compute_masks3d_gpu(dP, cp)
    assert m.dtype == torch.int32 and np.array_equal(m.numpy(), o["masks"])
    raw = gpu.follow_and_label3d((dP, cp))
    assert np.array_equal(raw.numpy(), ref.get_masks3d(o["p"], o["inds"], v["shape"]))
    hist, pos = cc.hist_pos(o["bins"], o["inds"], v["shape"])
    got = gpu.get_masks3d_gpu(torch.from_numpy(hist), torch.from_numpy(pos), v["shape"])
    assert np.array_equal(got.numpy(), raw.numpy())
    assert np.array_equal(gpu.fill_holes3d_gpu(raw, 15).numpy(), o["masks"])
    _, yx, zx, zy = _coded_views(3, 5, 7)
    acc = gpu.combine_views3d_gpu(*(torch.from_numpy(a) for a in (yx, zx, zy)))
    dPw, cpw = ref.combine_views3d(yx, zx, zy)
    assert np.array_equal(acc[:3].numpy(), dPw) and np.array_equal(acc[3].numpy(), cpw)
    with pytest.raises(ValueError, match="too large"):
        gpu._check_volume(1300, 1300, 1300)


# ------------------------------------------------------------------ runner


@pytest.fixture(scope="module")
def cpu_runner():
    from bioengine_worker_amd.cellpose.pipeline import CellposeRunner
    from bioengine_worker_amd.models.cpnet import CPnet

    return CellposeRunner(CPnet().randomize_(0), device="cpu")


def _fake_net(a, b, c):
    def run_net(x, p):
        x0 = x[:, 0]
        return torch.stack([a * x0, b * x0, c * x0], 1), torch.ones(x.shape[0], 4)

    return run_net


@pytest.mark.unit
def test_eval_3d_routes_three_views(cpu_runner, monkeypatch):
    monkeypatch.setattr(cpu_runner, "run_net", _fake_net(1.0, 2.0, 4.0))
    Z, H, W = 5, 7, 9
    vol = np.random.default_rng(0).integers(0, 50, (Z, H, W)).astype(np.float32)
    m, f, s = cpu_runner.eval_3d(vol, normalize=False, stack_batch=4, niter=5)
    assert m.shape == (Z, H, W) and m.dtype == torch.int32
    assert f.shape == (4, Z, H, W) and f.dtype == torch.float32 and s.shape == (4,)
    x = torch.from_numpy(vol)
    # (a, b, c) * x per plane -> dZ = 2a, dY = a + b, dX = 2b, cellprob = 3c, voxel for voxel
    assert torch.equal(f, torch.stack([2 * x, 3 * x, 4 * x, 12 * x]))
    assert torch.allclose(s, torch.ones(4))  # mean of the YX planes' styles
    # [Z, C, H, W] and channel-last layouts give the same field
    v4 = np.stack([vol, np.zeros_like(vol)], 1)
    assert torch.equal(cpu_runner.eval_3d(v4, normalize=False, niter=5)[1], f)
    assert torch.equal(cpu_runner.eval_3d(np.ascontiguousarray(v4.transpose(0, 2, 3, 1)), normalize=False, niter=5)[1], f)
    none, f2, _ = cpu_runner.eval_3d(vol, normalize=False, compute_masks=False)
    assert none is None and torch.equal(f2, f)


@pytest.mark.unit
def test_eval_3d_normalises_once_over_the_volume(cpu_runner, monkeypatch):
    monkeypatch.setattr(cpu_runner, "run_net", _fake_net(1.0, 2.0, 4.0))
    vol = np.random.default_rng(1).uniform(0, 1000, (5, 7, 9)).astype(np.float32)
    _, f, _ = cpu_runner.eval_3d(vol, compute_masks=False)
    xn = ref.normalize99(vol.reshape(1, 5 * 7, 9)).reshape(5, 7, 9)
    assert torch.equal(f[3], 12 * torch.from_numpy(xn))


@pytest.mark.unit
def test_eval_3d_masks_are_compute_masks3d(cpu_runner, monkeypatch):
    """A network that returns the capped flows of volume "b" for whatever plane it is shown."""
    v, o = cc.volume("b", "capped"), cc.oracle("b", "capped")
    Z, H, W = v["shape"]
    dP, cp = torch.from_numpy(v["dP"].copy()), torch.from_numpy(v["cellprob"].copy())
    calls = {"n": 0}

    def run_net(x, p):  # the planes arrive in order: YX (Z planes), ZX (H), ZY (W), whole views at once
        k = calls["n"]
        calls["n"] += 1
        if k == 0:
            y = torch.stack([dP[1], dP[2], cp], 1)  # [Z, 3, H, W]
        elif k == 1:
            y = torch.stack([dP[0], torch.zeros_like(cp), torch.zeros_like(cp)], 0).permute(2, 0, 1, 3)  # [H, 3, Z, W]
        else:
            y = torch.zeros(W, 3, Z, H)
        assert tuple(y.shape[2:]) == tuple(x.shape[2:]) and y.shape[0] == x.shape[0]
        return y.contiguous(), torch.ones(x.shape[0], 4)

    monkeypatch.setattr(cpu_runner, "run_net", run_net)
    m, f, _ = cpu_runner.eval_3d(np.zeros((Z, H, W), np.float32), normalize=False, stack_batch=64)
    assert calls["n"] == 3
    assert torch.equal(f[:3], dP) and torch.equal(f[3], cp)
    assert np.array_equal(m.numpy(), o["masks"]) and int(m.max()) == v["n"]


@pytest.mark.unit
def test_eval_3d_anisotropy(cpu_runner, monkeypatch):
    monkeypatch.setattr(cpu_runner, "run_net", _fake_net(1.0, 2.0, 4.0))
    Z, H, W = 5, 7, 9
    vol = np.random.default_rng(2).integers(0, 50, (Z, H, W)).astype(np.float32)
    m, f, _ = cpu_runner.eval_3d(vol, normalize=False, anisotropy=2.0, niter=5)
    assert m.shape == (Z, H, W) and m.dtype == torch.int32  # masks at the input depth
    assert f.shape == (4, 2 * Z, H, W)  # flows at the resampled depth
    xr = torch.nn.functional.interpolate(torch.from_numpy(vol)[None, None], size=(2 * Z, H, W), mode="trilinear",
                                         align_corners=False)[0, 0]
    assert torch.equal(f[3], 12 * xr)
    same, f1, _ = cpu_runner.eval_3d(vol, normalize=False, anisotropy=1.0, niter=5)
    assert f1.shape == (4, Z, H, W)
    with pytest.raises(ValueError, match="anisotropy"):
        cpu_runner.eval_3d(vol, anisotropy=0.0)
    with pytest.raises(ValueError, match="anisotropy"):
        cpu_runner.eval_3d(vol, anisotropy=-1.5)


@pytest.mark.unit
def test_eval_3d_anisotropy_nearest_plane_rule(cpu_runner, monkeypatch):
    """Masks come back by z_src = min(floor((z + 0.5) * Z' / Z), Z' - 1): checked on a volume whose
    resampled masks are known (volume "b" flows, handed out by a fake network at the resampled depth)."""
    from bioengine_worker_amd.cellpose import pipeline

    v, o = cc.volume("b", "capped"), cc.oracle("b", "capped")
    Zr, H, W = v["shape"]  # 19 planes after resampling 8 planes by 2.4 (round(19.2) = 19)
    Z = 8
    acc = np.concatenate([v["dP"], v["cellprob"][None]])
    monkeypatch.setattr(cpu_runner, "run_net", lambda x, p: (torch.zeros(x.shape[0], 3, *x.shape[2:]), torch.ones(x.shape[0], 4)))
    monkeypatch.setattr(pipeline.ref, "combine_views3d", lambda *a: (acc[:3], acc[3]))
    m, f, _ = cpu_runner.eval_3d(np.zeros((Z, H, W), np.float32), normalize=False, anisotropy=2.4)
    assert f.shape == (4, Zr, H, W) and m.shape == (Z, H, W)
    zs = [min(int(np.floor((z + 0.5) * Zr / Z)), Zr - 1) for z in range(Z)]
    want = o["masks"][zs]
    assert cc.match_fraction(m.numpy(), want) == 1.0 and int(m.max()) == len(np.unique(want)) - 1


@pytest.mark.unit
def test_eval_3d_rejects_bad_input(cpu_runner):
    with pytest.raises(ValueError, match="eval_3d expects"):
        cpu_runner.eval_3d(np.zeros((8, 8), np.float32))
    with pytest.raises(ValueError, match="at least"):
        cpu_runner.eval_3d(np.zeros((1, 16, 16), np.float32))
    with pytest.raises(ValueError, match="at least"):
        cpu_runner.eval_3d(np.zeros((4, 16, 16), np.float32), tile=False)


@pytest.mark.unit
def test_eval_3d_smallest_depth_runs_the_real_network(cpu_runner):
    from bioengine_worker_amd.cellpose.pipeline import CellposeRunner

    Z = CellposeRunner.MIN_DEPTH_3D
    vol = np.random.default_rng(3).uniform(0, 1, (Z, 9, 10)).astype(np.float32)
    m, f, s = cpu_runner.eval_3d(vol, niter=10)
    assert m.shape == (Z, 9, 10) and f.shape == (4, Z, 9, 10) and torch.isfinite(f).all() and s.dim() == 1


@pytest.mark.unit
def test_eval_and_eval_stack_ignore_anisotropy(cpu_runner):
    from bioengine_worker_amd.cellpose.pipeline import EvalParams, synthetic_cells

    assert EvalParams().anisotropy is None
    stack = synthetic_cells(2, 32, 32, ncells=3, seed=1)
    a = cpu_runner.eval(stack, flow_threshold=0.0)
    b = cpu_runner.eval(stack, EvalParams(anisotropy=2.0, flow_threshold=0.0))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    c = cpu_runner.eval_stack(stack, flow_threshold=0.0)
    d = cpu_runner.eval_stack(stack, anisotropy=3.0, flow_threshold=0.0)
    assert torch.equal(c[0], d[0]) and torch.equal(c[1], d[1])


# ------------------------------------------------------------------ app


@pytest.fixture()
def app(tmp_path, monkeypatch):
    from bioengine_worker_amd.compat import install

    install()
    monkeypatch.setenv("HOME", str(tmp_path))
    spec = importlib.util.spec_from_file_location("cellpose_main_3d_test", APP_MAIN)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.CellposeFinetune.func_or_class(default_model="cyto3")


@pytest.mark.unit
def test_app_do_3d(app):
    from bioengine_worker_amd.cellpose.pipeline import synthetic_cells

    vol = np.ascontiguousarray(synthetic_cells(6, 20, 24, ncells=3, seed=1)[:, 0])  # [Z, H, W] uint16
    kw = {"model": "cyto3", "niter": 20}

    async def main():
        a = await app.infer(input_arrays=[vol], do_3D=True, **kw)
        b = await app.infer(input_arrays=[np.ascontiguousarray(vol.transpose(1, 2, 0))], do_3D=True, z_axis=2, **kw)
        c = await app.infer({"input_arrays": [vol], "do_3D": True, "return_flows": True, "flow_threshold": 0.9, **kw})
        d = await app.infer({"input_arrays": [vol], "do_3D": True, "anisotropy": 1.5, "return_flows": True, **kw})
        j = await app.infer(input_arrays=[vol], do_3D=True, json_safe=True, **kw)
        with pytest.raises(ValueError, match="do_3D and stitch_threshold"):
            await app.infer(input_arrays=[vol], do_3D=True, stitch_threshold=0.25, **kw)
        with pytest.raises(ValueError, match="do_3D and stitch_threshold"):
            await app.infer({"input_arrays": [vol], "do_3D": True, "stitch_threshold": 0.25, **kw})
        with pytest.raises(ValueError, match="enable_clahe"):
            await app.infer(input_arrays=[vol], do_3D=True, enable_clahe=True, **kw)
        with pytest.raises(ValueError, match="anisotropy"):
            await app.infer(input_arrays=[vol], do_3D=True, anisotropy=0.0, **kw)
        with pytest.raises(ValueError, match="anisotropy"):
            await app.infer({"input_arrays": [vol], "do_3D": True, "anisotropy": -2.0, **kw})
        with pytest.raises(ValueError, match="z-stack"):
            await app.infer(input_arrays=[vol[0]], do_3D=True, **kw)
        plain = await app.infer(input_arrays=[vol[0]], flow_threshold=0.0, **kw)  # without do_3D: as before
        runner = await app._runner("cyto3")
        return a, b, c, d, j, plain, runner

    a, b, c, d, j, plain, runner = asyncio.run(asyncio.wait_for(main(), 600))
    out = a[0]["output"]
    assert out.shape == vol.shape and out.dtype == np.uint16 and a[0]["input_path"] == "input_arrays[0]"
    want, wf, _ = runner.eval_3d(vol, niter=20)
    assert np.array_equal(out, want.cpu().numpy())
    assert np.array_equal(b[0]["output"], out)  # z_axis moved
    assert np.array_equal(c[0]["output"], out)  # dict form; flow_threshold accepted and unused
    rgb, dp, cp = c[0]["flows"]
    assert rgb.shape == vol.shape + (3,) and rgb.dtype == np.uint8
    assert dp.shape == (3,) + vol.shape and cp.shape == vol.shape
    assert np.array_equal(dp, wf[:3].cpu().numpy()) and np.array_equal(cp, wf[3].cpu().numpy())
    assert d[0]["output"].shape == vol.shape
    assert d[0]["flows"][1].shape == (3, 9, 20, 24) and d[0]["flows"][0].shape == (9, 20, 24, 3)
    assert isinstance(j[0]["output"], list) and len(j[0]["output"]) == 6
    pm, _, _ = runner.eval(vol[0], flow_threshold=0.0, niter=20)
    assert plain[0]["output"].shape == (20, 24) and np.array_equal(plain[0]["output"], pm[0].cpu().numpy())
