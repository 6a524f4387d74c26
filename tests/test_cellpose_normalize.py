"""Cellpose normalisation options on the CPU: the parser (``pipeline.norm_params``), the oracle
(``reference.normalize_img`` and the stages of the tile normalisation), the runner's CPU path and the
app (``infer`` / ``start_training``)."""
import asyncio
import importlib.util
import json
import os
from pathlib import Path

import numpy as np
import pytest
import torch

from bioengine_worker_amd.cellpose import reference as ref
from bioengine_worker_amd.cellpose.pipeline import CellposeRunner, NormParams, norm_options, norm_params, synthetic_cells

ROOT = Path(__file__).resolve().parents[1]
APP_MAIN = ROOT / "apps" / "cellpose-finetuning" / "main.py"


# ---------------------------------------------------------------- parser

def test_norm_params_defaults_and_hash():
    d = NormParams()
    assert (d.normalize, d.lower, d.upper, d.lowhigh, d.invert, d.tile_blocksize) == (True, 1.0, 99.0, None, False, 0)
    defaults = {"lowhigh": None, "percentile": None, "normalize": True, "norm3D": True, "sharpen_radius": 0,
                "smooth_radius": 0, "tile_norm_blocksize": 0, "tile_norm_smooth3D": 1, "invert": False}
    for v in (True, {}, defaults, {"percentile": [1, 99]}, NormParams()):
        assert norm_params(v) == d and norm_params(v).is_default and norm_params(v).normalize
    off = norm_params(False)  # no normalisation: the other fields stay at their defaults
    assert off == NormParams(normalize=False) == norm_params({"normalize": False, "percentile": [2, 98]})
    assert not off.normalize and bool(off)  # truthiness says nothing about the switch: "given", not "on"
    a = norm_params({"percentile": [0.5, 99.5], "invert": True, "tile_norm_blocksize": 100.0})
    b = norm_params({"tile_norm_blocksize": 100, "invert": True, "percentile": (0.5, 99.5)})
    assert a == b == NormParams(True, 0.5, 99.5, None, True, 100) and hash(a) == hash(b) and len({a, b, d}) == 2
    assert norm_params({"lowhigh": [0, 4000]}).lowhigh == (0.0, 4000.0)
    assert norm_params({"lowhigh": [[0, 10], [5, 50.5]]}).lowhigh == ((0.0, 10.0), (5.0, 50.5))
    hash(norm_params({"lowhigh": [[0, 10], [5, 50.5]]}))
    assert norm_options({"norm3D": False}) == (d, False) and norm_options({"invert": True})[1] is None


@pytest.mark.parametrize("bad", [
    {"percentile": [99, 1]}, {"percentile": [-1, 99]}, {"percentile": [1, 100.5]}, {"percentile": [5, 5]},
    {"percentile": [1]}, {"lowhigh": [1.0, 1.0005]}, {"lowhigh": [[0, 1], [3, 2]]},
    {"lowhigh": [0, 1], "tile_norm_blocksize": 50}, {"tile_norm_blocksize": -3},
    {"sharpen_radius": 2}, {"smooth_radius": 1}, {"tile_norm_smooth3D": 0}, {"nonsense": 1},
    {"invert": True, "normalize": False}, {"tile_norm_blocksize": [100]}, {"smooth_radius": "a"}, {"tile_norm_blocksize": float("inf")},
    {"tile_norm_blocksize": float("nan")}, {"tile_norm_blocksize": True}, "yes", 3,
])
def test_norm_params_rejections(bad):
    with pytest.raises(ValueError):
        norm_params(bad)


def test_unsupported_options_say_so():
    with pytest.raises(ValueError, match="not supported"):
        norm_params({"sharpen_radius": 2})


# ---------------------------------------------------------------- oracle

def _ramp_image():
    """96 x 128 uint16 texture under a 5:1 illumination ramp along x."""
    rng = np.random.default_rng(0)
    ill = np.linspace(1.0, 0.2, 128)[None, :]
    return (100 + 4000 * ill * rng.random((96, 128)) ** 3).astype(np.uint16)[None]


def test_normalize_img_global_rules():
    img = synthetic_cells(1, 40, 52, ncells=5, seed=1)[0]  # [2, H, W] uint16
    assert np.array_equal(ref.normalize_img(img, NormParams()), ref.normalize99(img))
    assert np.array_equal(ref.normalize_img(img, norm_params({"percentile": [0.5, 99.5]})), ref.normalize99(img, 0.5, 99.5))
    inv = ref.normalize_img(img, norm_params({"invert": True}))
    assert inv.dtype == np.float32 and np.array_equal(inv, 1 - ref.normalize99(img))
    lh = ref.normalize_img(img, norm_params({"lowhigh": [[0, 1000], [10, 510]]}))
    x = img.astype(np.float32)
    assert np.array_equal(lh[0], x[0] / np.float32(1000)) and np.array_equal(lh[1], (x[1] - 10) / np.float32(500))
    both = ref.normalize_img(img, norm_params({"lowhigh": [10, 510]}))
    assert np.array_equal(both[0], (x[0] - 10) / np.float32(500)) and np.array_equal(both[1], lh[1])
    assert np.array_equal(ref.normalize_img(img, norm_params(False)), x)


@pytest.mark.parametrize("hw,bs,grid", [((70, 90), 32, (3, 4)), ((33, 47), 8, (5, 8)), ((300, 280), 256, (2, 2)),
                                         ((20, 90), 32, (1, 4)), ((32, 20), 32, (1, 1))])
def test_block_layout(hw, bs, grid):
    for L, n in zip(hw, grid):
        starts, b = ref.tile_norm_blocks(L, bs)
        assert len(starts) == n and b == min(bs, L) and starts[0] == 0 and starts[-1] == L - b
        assert starts == ref.tile_starts(L, bs, 0.1) and all(s1 - s0 <= b for s0, s1 in zip(starts, starts[1:]))
    x01, _ = ref.tile_norm_raw_maps(np.zeros((1,) + hw, np.uint8), bs)
    assert x01.shape == (1,) + grid


def test_degenerate_block_takes_nearest_valid_neighbour():
    img = _ramp_image()
    img[0, :32, :32] = 500  # exactly block (0, 0)
    x01, x99 = ref.tile_norm_raw_maps(img, 32)
    bad = (x99 - x01) < 1e-3
    assert bad.sum() == 1 and bad[0, 0, 0]
    f01, f99 = ref.tile_norm_fill(x01, x99)
    assert f01[0, 0, 0] == x01[0, 0, 1] and f99[0, 0, 0] == x99[0, 0, 1]  # (0, 1) before (1, 0) in raster order
    keep = ~bad
    assert np.array_equal(f01[keep], x01[keep]) and np.array_equal(f99[keep], x99[keep])
    assert np.isfinite(ref.normalize99_tile(img, 32)).all()


def test_fill_ties_go_to_the_raster_first_block():
    lo = np.full((1, 3, 3), 5.0, np.float32)
    hi = lo.copy()
    for k, (j, i) in enumerate(((0, 1), (1, 0), (1, 2), (2, 1))):
        lo[0, j, i], hi[0, j, i] = 10.0 * (k + 1), 10.0 * (k + 1) + 100.0 + k
    f01, f99 = ref.tile_norm_fill(lo, hi)
    want = {(0, 0): (0, 1), (1, 1): (0, 1), (0, 2): (0, 1), (2, 0): (1, 0), (2, 2): (1, 2)}
    for (j, i), (sj, si) in want.items():
        assert f01[0, j, i] == lo[0, sj, si] and f99[0, j, i] == hi[0, sj, si], (j, i)


def test_constant_channel_is_the_identity():
    img = np.stack([_ramp_image()[0], np.full((96, 128), 77, np.uint16)])
    x01, x99 = ref.tile_norm_maps(img, 32)
    assert not x01[1].any() and (x99[1] == 1).all()
    out = ref.normalize99_tile(img, 32)
    assert np.array_equal(out[1], img[1].astype(np.float32))
    assert np.array_equal(out[0], ref.normalize99_tile(img[:1], 32)[0])  # channels are independent


def test_blocksize_above_both_axes_is_the_global_rule():
    """One block: both maps are one cell, and smoothing and enlarging a one-cell map keep its value
    up to one float32 rounding (nine weights that sum to 1 within float64 rounding).  What is left
    between the two rules is the rounding of lo and hi: with each moved by at most half a float32
    ulp (eps = 2**-24 relative), (x - lo) / (hi - lo) moves by at most
    eps * (|lo| + (|lo| + |hi|) * max|x - lo| / (hi - lo)) / (hi - lo), plus one rounding of the
    result, eps * max|result|.  For this image (values 100..4100, hi - lo ~ 2900) that is 1.6e-7."""
    img = _ramp_image()
    g, t = ref.normalize99(img), ref.normalize99_tile(img, 256)
    x = img.astype(np.float64)
    lo, hi = np.percentile(x, 1), np.percentile(x, 99)
    eps = 2.0 ** -24
    bound = eps * (abs(lo) + (abs(lo) + abs(hi)) * np.abs(x - lo).max() / (hi - lo)) / (hi - lo) + eps * np.abs(g).max()
    err = float(np.abs(g - t).max())
    print(f"one block vs global: {err:.3e}, bound {bound:.3e}")
    assert err <= bound < 1e-6
    assert ref.tile_norm_maps(img, 256)[0].shape == (1, 1, 1)


def test_tile_norm_evens_out_an_illumination_ramp():
    """Quadrant 99th percentiles of the normalised image, max / min: measured here 1.77 under the
    global rule and 1.19 under tile normalisation at blocksize 32 (ramp along x, so the left and
    right quadrants differ).  Asserted: the order, with a margin of 0.2 between the two ratios."""
    img = _ramp_image()

    def spread(x):
        q = [np.percentile(x[0, ys, xs], 99) for ys in (slice(0, 48), slice(48, 96)) for xs in (slice(0, 64), slice(64, 128))]
        return max(q) / min(q)

    g, t = spread(ref.normalize99(img)), spread(ref.normalize_img(img, norm_params({"tile_norm_blocksize": 32})))
    print(f"quadrant p99 max/min: global {g:.3f}, tile {t:.3f}")
    assert 1.0 <= t < g - 0.2


def test_normalize_img_gpu_on_cpu_tensors_follows_the_oracle():
    """``gpu.normalize_img_gpu`` on CPU tensors (the path a CPU session takes through the same call):
    ``normalize=False`` converts only, every other rule is the oracle's."""
    from bioengine_worker_amd.cellpose.gpu import normalize_img_gpu

    x = torch.from_numpy(synthetic_cells(2, 40, 52, ncells=5, seed=1).astype(np.int32)).to(torch.float32)
    off = normalize_img_gpu(x, NormParams(normalize=False))
    assert off.dtype == torch.float32 and torch.equal(off, x) and float(off.max()) > 100
    assert torch.equal(normalize_img_gpu(x, norm_params(False), c_use=1), x[:, :1])
    for opt in ({"invert": True}, {"tile_norm_blocksize": 16}, {"lowhigh": [0, 1000]}):
        P = norm_params(opt)
        want = np.stack([ref.normalize_img(x[b].numpy(), P) for b in range(2)])
        assert np.array_equal(normalize_img_gpu(x, P).numpy(), want)
    assert float(normalize_img_gpu(x).max()) < 10  # None is the default rule


def test_option_caches_are_bounded():
    from bioengine_worker_amd.cellpose import gpu as cg

    cache = cg.collections.OrderedDict()
    for k in range(3 * cg._CONST_CACHE_MAX):
        assert cg._cached_const(cache, k, lambda k=k: k * 2) == k * 2
    assert len(cache) == cg._CONST_CACHE_MAX and next(iter(cache)) == 2 * cg._CONST_CACHE_MAX
    cg._cached_const(cache, 2 * cg._CONST_CACHE_MAX, lambda: None)  # a hit moves the entry to the young end
    assert next(reversed(cache)) == 2 * cg._CONST_CACHE_MAX


def test_constants_a_recording_holds_outlive_their_eviction():
    """What a captured HIP graph keeps (``gpu.norm_constants``, stored in the runner's graph entry):
    the tensors stay what they were after more than a cache's worth of other keys went in, and a
    new lookup builds new objects, which is how the runner notices an eviction during a capture."""
    from bioengine_worker_amd.cellpose import gpu as cg

    P = NormParams(tile_blocksize=32)
    L = NormParams(lowhigh=((3.0, 200.0), (-5.0, 90.5)))
    keep = cg.norm_constants(P, 2, 70, 90, "cpu") + cg.norm_constants(L, 2, 70, 90, "cpu")
    assert len(keep) == 3 and all(a is b for a, b in zip(keep, cg.norm_constants(P, 2, 70, 90, "cpu") +
                                                         cg.norm_constants(L, 2, 70, 90, "cpu")))
    assert cg.norm_constants(NormParams(), 2, 70, 90, "cpu") == () == cg.norm_constants(NormParams(normalize=False), 2, 70, 90, "cpu")
    want = [t.clone() for t in keep]
    for k in range(cg._CONST_CACHE_MAX + 6):
        cg.norm_constants(NormParams(tile_blocksize=32), 2, 100 + k, 90, "cpu")
        cg.norm_constants(NormParams(lowhigh=(0.0, 10.0 + k)), 2, 70, 90, "cpu")
    assert len(cg._tile_norm_grids) == len(cg._lowhigh_consts) == cg._CONST_CACHE_MAX
    assert (70, 90, 32, torch.device("cpu")) not in cg._tile_norm_grids  # evicted ...
    assert all(torch.equal(a, b) for a, b in zip(keep, want))  # ... and still whole for its holder
    assert keep[0].tolist() == ref.tile_norm_blocks(70, 32)[0] and keep[1].tolist() == ref.tile_norm_blocks(90, 32)[0]
    again = cg.norm_constants(P, 2, 70, 90, "cpu") + cg.norm_constants(L, 2, 70, 90, "cpu")
    assert not any(a is b for a, b in zip(keep, again)) and all(torch.equal(a, b) for a, b in zip(keep, again))


# ---------------------------------------------------------------- runner, CPU path

@pytest.fixture(scope="module")
def runner():
    return CellposeRunner(device="cpu", seed=0)


def _ramped_cells(n, H, W, seed):
    ill = np.linspace(1.0, 0.3, W)[None, None, None, :]
    return (synthetic_cells(n, H, W, ncells=6, seed=seed) * ill).astype(np.uint16)


def test_eval_on_the_cpu_uses_the_oracle(runner):
    from bioengine_worker_amd.cellpose.pipeline import EvalParams

    imgs = _ramped_cells(2, 40, 52, 1)
    opt = {"tile_norm_blocksize": 16, "invert": True}
    P = norm_params(opt)
    x = torch.stack([torch.from_numpy(ref.normalize_img(im, P)) for im in imgs])
    want_y, want_s = runner.run_net(x, EvalParams(bsize=32))
    _, y, s = runner.eval(imgs, bsize=32, normalize=dict(opt), compute_masks=False)
    assert torch.equal(y, want_y) and torch.equal(s, want_s)
    _, y0, _ = runner.eval(imgs, bsize=32, compute_masks=False)
    assert not torch.equal(y0, y)
    _, yp, _ = runner.eval(imgs, bsize=32, normalize=P, compute_masks=False)  # the canonical form is taken too
    assert torch.equal(yp, y)
    # a stack whose planes are normalised one by one goes the same way
    _, ys, _ = runner.eval_stack(imgs, bsize=32, normalize={**opt, "norm3D": False}, compute_masks=False)
    assert torch.equal(ys, y)
    _, ys2, _ = runner.eval_stack(imgs, bsize=32, normalize=dict(opt), norm3d=False, compute_masks=False)
    assert torch.equal(ys2, y)


def test_stack_wide_rules_take_percentile_lowhigh_invert(runner):
    from bioengine_worker_amd.cellpose.pipeline import EvalParams

    vol = _ramped_cells(3, 24, 28, 2)  # [Z, C, H, W]
    P = norm_params({"percentile": [2, 98], "invert": True})
    whole = ref.normalize_img(vol.transpose(1, 0, 2, 3).reshape(2, 3 * 24, 28), P).reshape(2, 3, 24, 28).transpose(1, 0, 2, 3)
    want, _ = runner.run_net(torch.from_numpy(np.ascontiguousarray(whole)), EvalParams(bsize=32))
    _, y, _ = runner.eval_stack(vol, bsize=32, normalize={"percentile": [2, 98], "invert": True}, compute_masks=False)
    assert torch.equal(y, want)


def test_tile_norm_over_a_volume_raises(runner):
    vol = _ramped_cells(8, 16, 16, 3)[:, 0]
    with pytest.raises(ValueError, match="tile_norm_blocksize"):
        runner.eval_3d(vol, normalize={"tile_norm_blocksize": 8})
    with pytest.raises(ValueError, match="tile_norm_blocksize"):
        runner.eval_stack(vol, normalize={"tile_norm_blocksize": 8})  # norm3D defaults to True
    with pytest.raises(ValueError, match="not supported"):
        runner.eval(vol[:1], normalize={"smooth_radius": 3})


# ---------------------------------------------------------------- app

@pytest.fixture()
def app(tmp_path, monkeypatch):
    from bioengine_worker_amd.compat import install

    install()
    monkeypatch.setenv("HOME", str(tmp_path))
    spec = importlib.util.spec_from_file_location("cellpose_main_normalize_test", APP_MAIN)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.CellposeFinetune.func_or_class(default_model="cyto3")


@pytest.fixture()
def evals(monkeypatch):
    """Every network stage as (images in the batch, its canonical ``normalize``)."""
    from bioengine_worker_amd.cellpose import pipeline

    seen = []
    real = pipeline.CellposeRunner.run_net

    def spy(self, x, p, *args, **kw):
        seen.append((int(x.shape[0]), norm_params(p.normalize)))
        return real(self, x, p, *args, **kw)

    monkeypatch.setattr(pipeline.CellposeRunner, "run_net", spy)
    return seen


def test_app_infer_with_normalize(app, evals):
    imgs = synthetic_cells(2, 48, 56, ncells=6, seed=2)
    kw = {"model": "cyto3", "niter": 20, "flow_threshold": 0.0}
    inv = NormParams(invert=True)

    async def main():
        on = await app.infer(input_arrays=[imgs[0]], normalize={"invert": True}, return_flows=True, **kw)
        solo = list(evals)
        d = await app.infer({"input_arrays": [imgs[0]], "normalize": {"invert": True}, "return_flows": True, **kw})
        off = await app.infer(input_arrays=[imgs[0]], return_flows=True, **kw)
        del evals[:]
        mixed = await asyncio.gather(app.infer(input_arrays=[imgs[0]], normalize={"invert": True}, return_flows=True, **kw),
                                     app.infer(input_arrays=[imgs[0]], normalize=True, return_flows=True, **kw))
        apart = list(evals)
        del evals[:]
        await asyncio.gather(app.infer(input_arrays=[imgs[0]], normalize={"invert": True}, **kw),
                             app.infer(input_arrays=[imgs[1]], normalize={"invert": True, "percentile": [1, 99]}, **kw))
        together = list(evals)
        e = await app.evaluate(input_arrays=[imgs[0]], label_arrays=[np.zeros((48, 56), np.int32)],
                               normalize={"tile_norm_blocksize": 24}, **kw)
        return on, solo, d, off, mixed, apart, together, e

    on, solo, d, off, mixed, apart, together, e = asyncio.run(asyncio.wait_for(main(), 600))
    assert solo == [(1, inv)]
    assert np.array_equal(d[0]["flows"][1], on[0]["flows"][1])
    assert not np.array_equal(on[0]["flows"][1], off[0]["flows"][1])  # the option reaches the network stage
    assert sorted(apart, key=lambda t: t[1].invert) == [(1, NormParams()), (1, inv)]  # never one batch
    assert np.array_equal(mixed[0][0]["flows"][1], on[0]["flows"][1])
    assert np.array_equal(mixed[1][0]["flows"][1], off[0]["flows"][1])
    assert together == [(2, inv)]  # equal options, however spelled, share a batch
    assert evals[-1] == (1, NormParams(tile_blocksize=24)) and len(e["per_image"]) == 1

    async def bad():
        await app.infer(input_arrays=[imgs[0]], normalize={"sharpen_radius": 3}, **kw)

    with pytest.raises(ValueError, match="not supported"):
        asyncio.run(bad())


def test_session_normalize_is_stored_and_becomes_the_default(app, evals, monkeypatch):
    from bioengine_worker_amd.train import session

    preps = []
    real = session._prep

    def spy(imgs, labs, device, normalize=True):
        preps.append(normalize)
        return real(imgs, labs, device, normalize)

    monkeypatch.setattr(session, "_prep", spy)
    from bioengine_worker_amd.train.cellpose_train import synthetic_instances

    ims, labs = synthetic_instances(2, 64, 64, ncells=6, seed=3)
    arrs = [(im[0] * 1000 + 200).astype(np.uint16) for im in ims]
    opt = {"percentile": [0.5, 99.5], "invert": True}

    async def main():
        with pytest.raises(ValueError):
            await app.start_training(train_arrays=arrs[:1], label_arrays=[labs[0]], model="cyto3", normalize={"bogus": 1})
        r = await app.start_training(train_arrays=arrs[:1], label_arrays=[labs[0]], test_arrays=arrs[1:],
                                     test_label_arrays=[labs[1]], model="cyto3", n_epochs=1, min_train_masks=1,
                                     normalize=dict(opt))
        sid = r["session_id"]
        for _ in range(2400):
            st = await app.get_training_status(session_id=sid)
            if st["status_type"] in ("completed", "failed", "stopped"):
                break
            await asyncio.sleep(0.05)
        del evals[:]
        await app.infer(input_arrays=[arrs[0]], model=sid, niter=20)
        inherited = list(evals)
        del evals[:]
        await app.infer(input_arrays=[arrs[0]], model=sid, niter=20, normalize=True)
        return sid, st, inherited, list(evals)

    sid, st, inherited, explicit = asyncio.run(asyncio.wait_for(main(), 600))
    assert st["status_type"] == "completed", st
    stored = json.loads((Path(os.environ["HOME"]) / "sessions" / sid / "training_params.json").read_text())
    assert stored["normalize"] == opt
    assert preps == [opt, opt]  # training and test images
    assert inherited == [(1, norm_params(opt))] and explicit == [(1, NormParams())]
