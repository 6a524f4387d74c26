"""Cellpose normalisation options on the GPU: block percentiles, the maps (fill + smoothing), the
unfused apply and the normalising gather, against the numpy oracle (``reference.normalize_img`` and
its stages) and against each other.  Data kinds as in ``test_cellpose_frontend.py``."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.int16)


def _data(shape, kind, seed=0):
    g = torch.Generator().manual_seed(seed)
    if kind == "uint8":
        return (torch.rand(shape, generator=g) ** 3 * 255).round().to(torch.uint8)
    if kind == "uint16":  # microscopy-like: many ties, a dominant background mode
        return (torch.rand(shape, generator=g) ** 4 * 4000).round().to(torch.int32).to(torch.uint16)
    return torch.randn(shape, generator=g) * 100  # float32 with negative values


def _np(x):
    return x.to(torch.int32).numpy() if x.dtype == torch.uint16 else x.numpy()


KINDS = ["uint8", "uint16", "float32"]

# ---------------------------------------------------------------- block percentiles

BLOCK_CASES = {
    "multi": dict(shape=(2, 2, 70, 90), bs=32, c_use=2),
    "odd": dict(shape=(1, 1, 33, 47), bs=8, c_use=1),  # odd row stride, unaligned rectangle rows
    "short": dict(shape=(1, 1, 20, 90), bs=32, c_use=1),  # one block row shorter than the blocksize
    "wide": dict(shape=(2, 3, 70, 90), bs=32, c_use=2),  # the third channel is ignored
}


def _check_blocks(x, bs, c_use, pct, gpu):
    """Against np.percentile of the same float32 blocks: exact where both ranks of a percentile hold
    one value, otherwise within 4 * 2**-24 * max(|a|, |b|) of the two order statistics a, b: three
    fp32 roundings of a*(1-f) + b*f plus one for a contracted multiply-add.  np.percentile is given
    the block's float32 values widened to float64: on a float32 array numpy also rounds the
    fractional rank q * (n - 1) / 100 to float32, an error of its own of up to ~n * 2**-24 * (b - a)
    (7.6e-5 at 245.08 in a 32 x 32 block of uint8 pixels) that has nothing to do with the kernel."""
    from bioengine_worker_amd.cellpose import gpu as cg
    from bioengine_worker_amd.cellpose import reference as ref

    B, C, H, W = x.shape
    lo, hi = cg.tile_block_percentiles_gpu(x.to(gpu), bs, *pct, c_use=c_use)
    ys, bh = ref.tile_norm_blocks(H, bs)
    xs, bw = ref.tile_norm_blocks(W, bs)
    assert lo.shape == hi.shape == (B, c_use, len(ys), len(xs))
    lo, hi = lo.cpu().numpy(), hi.cpu().numpy()
    xn = _np(x)
    n = bh * bw
    worst = 0.0
    for b in range(B):
        for c in range(c_use):
            for j, y0 in enumerate(ys):
                for i, x0 in enumerate(xs):
                    blk = xn[b, c, y0: y0 + bh, x0: x0 + bw].astype(np.float32)
                    srt = np.sort(blk.ravel())
                    for q, got in ((pct[0], lo[b, c, j, i]), (pct[1], hi[b, c, j, i])):
                        k = int(q / 100.0 * (n - 1))
                        a, bb = float(srt[k]), float(srt[min(k + 1, n - 1)])
                        want = float(np.percentile(blk.astype(np.float64), q))
                        if a == bb:
                            assert got == a == want, (b, c, j, i, q)
                        else:
                            tol = 4 * 2.0 ** -24 * max(abs(a), abs(bb))
                            worst = max(worst, abs(float(got) - want) / tol)
                            assert abs(float(got) - want) <= tol, (b, c, j, i, q, got, want, tol)
    print(f"block percentiles: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", list(BLOCK_CASES))
def test_block_percentiles_match_numpy(gpu, case, kind):
    cfg = BLOCK_CASES[case]
    _check_blocks(_data(cfg["shape"], kind), cfg["bs"], cfg["c_use"], (1.0, 99.0), gpu)


def test_block_percentiles_other_percentiles_and_ties(gpu):
    x = _data((1, 1, 70, 90), "uint16", seed=4)
    x[0, 0, :32, :32] = 1234  # a constant block: both ranks of both percentiles on one value
    _check_blocks(x, 32, 1, (0.5, 99.5), gpu)
    _check_blocks(x, 32, 1, (0.0, 100.0), gpu)


def test_block_larger_than_lds(gpu):
    """A 256 x 256 float32 block is 256 KiB, more than a CU's LDS: the select never holds a block there."""
    _check_blocks(_data((1, 1, 300, 280), "float32", seed=5), 256, 1, (1.0, 99.0), gpu)


# ---------------------------------------------------------------- maps: fill + smoothing

def _map_inputs():
    """Raw block maps [C, ny, nx] float32 for the three fill rules."""
    from bioengine_worker_amd.cellpose import reference as ref

    rng = np.random.default_rng(0)
    img = (100 + 4000 * rng.random((2, 96, 128)) ** 3).astype(np.uint16)
    one = img.copy()
    one[0, :32, :32] = 500  # exactly block (0, 0) of channel 0
    const = img.copy()
    const[1] = 77  # a channel without any valid block
    out = {"one_block": ref.tile_norm_raw_maps(one, 32), "const_channel": ref.tile_norm_raw_maps(const, 32)}
    assert int(((out["one_block"][1] - out["one_block"][0]) < 1e-3).sum()) == 1
    # ties: only the four edge-centre cells of a 3 x 3 grid are valid, with distinct values; the
    # centre and every corner are equally far from two or four of them
    lo = np.full((1, 3, 3), 5.0, np.float32)
    hi = lo.copy()
    for k, (j, i) in enumerate(((0, 1), (1, 0), (1, 2), (2, 1))):
        lo[0, j, i], hi[0, j, i] = 10.0 * (k + 1), 10.0 * (k + 1) + 100.0 + k
    out["ties"] = (lo, hi)
    # the largest grid the maps kernel holds (64 x 64 = 4096 cells), a tenth of it degenerate
    lo = (rng.random((1, 64, 64)) * 100).astype(np.float32)
    hi = lo + (1 + rng.random((1, 64, 64)) * 1000).astype(np.float32)
    hi[rng.random((1, 64, 64)) < 0.1] = 0
    hi = np.maximum(hi, lo)
    out["limit_grid"] = (lo, hi)
    return out


@pytest.mark.parametrize("name", ["one_block", "const_channel", "ties", "limit_grid"])
def test_maps_fill_and_smooth_match_the_oracle(gpu, name):
    """Tolerance: 4 x the largest difference between the oracle's map stage (fill + smoothing) run
    in float32 and in float64 numpy on the same raw maps.  Measured on the CPU: 1.6e-4 (one_block),
    1.4e-4 (const_channel), 4.7e-6 (ties), 5.4e-5 (limit_grid): the rounding of float32 results of up to
    ~4000, ~130 and ~1100."""
    from bioengine_worker_amd.cellpose import gpu as cg
    from bioengine_worker_amd.cellpose import reference as ref

    lo, hi = _map_inputs()[name]
    w32 = [ref.tile_norm_smooth(m) for m in ref.tile_norm_fill(lo, hi)]
    w64 = [ref.tile_norm_smooth(m) for m in ref.tile_norm_fill(lo.astype(np.float64), hi.astype(np.float64))]
    measured = max(float(np.abs(a - b).max()) for a, b in zip(w32, w64))
    print(f"maps {name}: oracle float32 vs float64 = {measured:.3e}")
    assert measured > 0
    g_lo, g_hi = cg.tile_maps_fill_smooth_gpu(torch.from_numpy(lo)[None].to(gpu), torch.from_numpy(hi)[None].to(gpu))
    for got, want in ((g_lo, w32[0]), (g_hi, w32[1])):
        err = float(np.abs(got[0].cpu().numpy().astype(np.float64) - want).max())
        print(f"maps {name}: gpu vs oracle = {err:.3e}")
        assert err <= 4 * measured
    if name == "const_channel":
        assert float(g_lo[0, 1].abs().max()) <= 4 * measured and float((g_hi[0, 1] - 1).abs().max()) <= 4 * measured
    if name == "ties":  # before smoothing, through the oracle's helper: centre and corner (0, 0) take block (0, 1)
        f_lo, f_hi = ref.tile_norm_fill(lo, hi)
        assert f_lo[0, 1, 1] == f_lo[0, 0, 0] == lo[0, 0, 1] and f_hi[0, 1, 1] == hi[0, 0, 1]


def test_grid_too_large_raises_and_leaves_nothing_behind(gpu):
    from bioengine_worker_amd.cellpose import gpu as cg

    big = torch.zeros(1, 1, 300, 300, dtype=torch.uint8, device=gpu)  # blocksize 4: 90 x 90 = 8100 blocks
    with pytest.raises(ValueError, match="4096"):
        cg.tile_norm_maps_gpu(big, 4)
    with pytest.raises(ValueError, match="4096"):
        cg.TilePlan(300, 300, 32, 0.1, device=gpu).gather_normalized(big, 8, 1, params=_P(tile_blocksize=4))
    with pytest.raises(ValueError, match="4096"):
        cg.tile_maps_fill_smooth_gpu(torch.zeros(1, 1, 65, 64, device=gpu), torch.ones(1, 1, 65, 64, device=gpu))
    _check_blocks(_data((1, 1, 70, 90), "uint16"), 32, 1, (1.0, 99.0), gpu)


# ---------------------------------------------------------------- fused against unfused

def _P(**kw):
    from bioengine_worker_amd.cellpose.pipeline import NormParams

    return NormParams(**kw)


PARAMS = {
    "tile": dict(tile_blocksize=32),
    "tile_invert": dict(tile_blocksize=32, invert=True),
    "lowhigh": dict(lowhigh=((3.0, 200.0), (-5.0, 90.5))),
    "pct_invert": dict(lower=0.5, upper=99.5, invert=True),
}


@pytest.mark.parametrize("augment", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pname", list(PARAMS))
def test_fused_gather_equals_unfused(gpu, pname, kind, augment):
    from bioengine_worker_amd.cellpose import gpu as cg

    P = _P(**PARAMS[pname])
    x = _data((3, 2, 70, 90), kind, seed=1).to(gpu)
    plan = cg.TilePlan(70, 90, 32, 0.1, device=gpu, augment=augment)
    want = plan.gather(cg.normalize_img_gpu(x, P), 8)
    got = plan.gather_normalized(x, 8, 2, params=P)
    assert got.shape == (3 * plan.nt, plan.by, plan.bx, 8) and got.dtype == torch.bfloat16
    assert torch.equal(_bits(got), _bits(want))
    assert got[..., :2].float().abs().max() > 0 and not got[..., 2:].any()  # channel padding is zero
    assert torch.equal(_bits(plan.gather_normalized(x, 8, 2, params=P)), _bits(got))  # two calls, identical bits
    # cpad of two 8-channel groups: the second group is all padding
    assert torch.equal(_bits(plan.gather_normalized(x, 16, 2, params=P)), _bits(plan.gather(cg.normalize_img_gpu(x, P), 16)))
    if kind != "float32":  # the raw integers and their float32 copy are the same pixels
        assert torch.equal(_bits(plan.gather_normalized(x.float(), 8, 2, params=P)), _bits(got))


@pytest.mark.parametrize("kind", KINDS)
def test_third_channel_is_ignored(gpu, kind):
    from bioengine_worker_amd.cellpose import gpu as cg

    P = _P(tile_blocksize=32)
    x = _data((2, 3, 70, 90), kind, seed=2).to(gpu)
    plan = cg.TilePlan(70, 90, 32, 0.1, device=gpu)
    got = plan.gather_normalized(x, 8, 2, params=P)
    assert torch.equal(_bits(got), _bits(plan.gather_normalized(x[:, :2].contiguous(), 8, 2, params=P)))
    assert not got[..., 2:].any()


@pytest.mark.parametrize("augment", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_default_params_are_todays_call(gpu, kind, augment):
    from bioengine_worker_amd.cellpose import gpu as cg

    x = _data((3, 2, 70, 90), kind, seed=3).to(gpu)
    plan = cg.TilePlan(70, 90, 32, 0.1, device=gpu, augment=augment)
    base = plan.gather_normalized(x, 8, 2)
    assert torch.equal(_bits(plan.gather_normalized(x, 8, 2, params=_P())), _bits(base))
    assert torch.equal(_bits(plan.gather_normalized(x, 8, 2, params=_P(lower=0.5, upper=99.5))),
                       _bits(plan.gather_normalized(x, 8, 2, 0.5, 99.5)))


# ---------------------------------------------------------------- unfused image against the oracle

@pytest.mark.parametrize("kind", KINDS)
def test_unfused_tile_norm_matches_the_oracle(gpu, kind):
    """``normalize_img_gpu`` against ``normalize99_tile`` on inputs whose block ranges span far more
    than 16 grey levels.  Tolerance: 4 x the largest difference between the oracle run in float32
    and in float64 on the same image.  Measured on the CPU: 1.8e-7 (uint8), 2.1e-7 (uint16), 4.6e-7 (float32),
    on results of magnitude up to 1.04 / 1.05 / 1.39."""
    from bioengine_worker_amd.cellpose import gpu as cg
    from bioengine_worker_amd.cellpose import reference as ref

    x = _data((2, 2, 70, 90), kind, seed=6)
    xn = _np(x)
    for b in range(2):
        lo, hi = ref.tile_norm_raw_maps(xn[b], 32)
        assert float((hi - lo).min()) >= 16
    w32 = np.stack([ref.normalize99_tile(xn[b], 32) for b in range(2)])
    w64 = np.stack([ref.normalize99_tile(xn[b], 32, dtype=np.float64) for b in range(2)])
    measured = float(np.abs(w32 - w64).max())
    got = cg.normalize_img_gpu(x.to(gpu), _P(tile_blocksize=32))
    assert got.dtype == torch.float32 and got.shape == x.shape
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - w32).max())
    print(f"unfused {kind}: oracle float32 vs float64 = {measured:.3e}, gpu vs oracle = {err:.3e}")
    assert measured > 0 and err <= 4 * measured
    inv = cg.normalize_img_gpu(x.to(gpu), _P(tile_blocksize=32, invert=True))
    assert torch.equal(inv, 1.0 - got)


def test_unfused_global_rules_match_the_oracle(gpu):
    """Fixed bounds and the inverted percentile rule against ``reference.normalize_img``: one fp32
    subtraction and one division on each side, on the same operands up to the percentile's own
    interpolation (4 * 2**-24 relative, as for the block percentiles) -> 1e-5 at |x| <= ~2."""
    from bioengine_worker_amd.cellpose import gpu as cg
    from bioengine_worker_amd.cellpose import reference as ref

    x = _data((2, 2, 70, 90), "uint16", seed=7)
    for P in (_P(lowhigh=((3.0, 200.0), (10.0, 3000.0))), _P(lowhigh=(0.0, 4000.0)), _P(lower=0.5, upper=99.5, invert=True)):
        want = np.stack([ref.normalize_img(_np(x)[b], P) for b in range(2)])
        got = cg.normalize_img_gpu(x.to(gpu), P).cpu().numpy()
        assert np.abs(got - want).max() <= 1e-5 * max(1.0, float(np.abs(want).max()))


# ---------------------------------------------------------------- training: images prepared on the device

@pytest.mark.parametrize("normalize", [False, True, {"percentile": [0.5, 99.5], "invert": True}, {"tile_norm_blocksize": 32},
                                       {"normalize": False}])
def test_session_prep_on_the_device_matches_the_oracle(gpu, normalize):
    """``train.session._prep`` on a GPU against ``reference.normalize_img`` of the same images.
    ``normalize`` off: the pixels as float32, exactly.  Tile normalisation: 4 x the oracle's own
    float32 / float64 difference on these images (measured on the CPU: 2.3e-7 and 2.1e-7).  The global rules:
    1e-5 relative to the largest value, as in ``test_unfused_global_rules_match_the_oracle``."""
    from bioengine_worker_amd.cellpose import reference as ref
    from bioengine_worker_amd.cellpose.pipeline import norm_params
    from bioengine_worker_amd.train.cellpose_train import synthetic_instances
    from bioengine_worker_amd.train.session import _prep

    _, labs = synthetic_instances(2, 70, 90, ncells=6, seed=3)
    imgs = [_np(_data((2, 70, 90), "uint16", seed=8 + k)).astype(np.uint16) for k in range(2)]
    xs, ys = _prep(imgs, list(labs), gpu, normalize)
    P = norm_params(normalize)
    assert len(xs) == len(ys) == 2
    for im, x in zip(imgs, xs):
        assert x.is_cuda and x.dtype == torch.float32 and x.shape == im.shape
        want = ref.normalize_img(im, P)
        got = x.cpu().numpy()
        if not P.normalize:
            assert np.array_equal(got, im.astype(np.float32)) and got.max() > 100
        elif P.tile_blocksize:
            measured = float(np.abs(want - ref.normalize99_tile(im, 32, dtype=np.float64)).max())
            err = float(np.abs(got.astype(np.float64) - want).max())
            print(f"_prep tile norm: oracle float32 vs float64 = {measured:.3e}, gpu vs oracle = {err:.3e}")
            assert measured > 0 and err <= 4 * measured
        else:
            assert np.abs(got - want).max() <= 1e-5 * max(1.0, float(np.abs(want).max()))


# ---------------------------------------------------------------- end to end

def _spy_calls(monkeypatch):
    from bioengine_worker_amd.ops import _native

    names = []
    real = _native.call

    def call(name, *args):
        names.append(name)
        return real(name, *args)

    monkeypatch.setattr(_native, "call", call)
    return names


def test_eval_fused_equals_unfused_and_differs_from_default(gpu, monkeypatch):
    from bioengine_worker_amd.cellpose import gpu as cg
    from bioengine_worker_amd.cellpose.pipeline import CellposeRunner

    runner = CellposeRunner(device=gpu, seed=0)
    rng = np.random.default_rng(0)
    ill = np.linspace(1.0, 0.2, 90)[None, None, None, :]
    x = torch.from_numpy((100 + 4000 * ill * rng.random((4, 2, 70, 90)) ** 3).astype(np.uint16)).to(gpu)
    opt = {"tile_norm_blocksize": 32}
    names = _spy_calls(monkeypatch)
    fused = runner.eval(x, bsize=32, normalize=dict(opt))
    assert "be_tiles_gather_tilenorm" in names and "be_pct_normalize_tile" not in names
    del names[:]
    host = runner.eval(x.float().cpu().numpy(), bsize=32, normalize=dict(opt))
    monkeypatch.setattr(cg, "FUSED_FRONT", False)
    del names[:]
    unfused = runner.eval(x, bsize=32, normalize=dict(opt))
    assert "be_pct_normalize_tile" in names and "be_tiles_gather_tilenorm" not in names
    monkeypatch.setattr(cg, "FUSED_FRONT", True)
    for other in (host, unfused):
        assert torch.equal(fused[0], other[0]) and torch.equal(fused[1], other[1])
    assert fused[0].shape == (4, 70, 90) and torch.isfinite(fused[1]).all()
    default = runner.eval(x, bsize=32)
    assert not torch.equal(default[1], fused[1])
    inverted = runner.eval(x, bsize=32, normalize={"invert": True})
    assert not torch.equal(inverted[1], default[1])


@pytest.mark.parametrize("opt", [{"lowhigh": [[3, 2000], [5, 900.5]]}, {"tile_norm_blocksize": 32}])
def test_graph_replay_after_its_constants_left_the_caches(gpu, opt):
    """A captured network stage records the addresses of the options' cached device constants.  The
    graph entry holds those tensors, so a replay after more than a cache's worth of other keys
    went in reads what it read at capture and equals the eager result."""
    from bioengine_worker_amd.cellpose import gpu as cg
    from bioengine_worker_amd.cellpose.pipeline import CellposeRunner, NormParams, norm_params

    runner = CellposeRunner(device=gpu, seed=0)
    x = _data((2, 2, 70, 90), "uint16", seed=9).to(gpu)
    kw = dict(bsize=32, compute_masks=False)
    _, want, want_s = runner.eval(x, normalize=dict(opt), **kw)
    runner.GRAPH_NET_MAX_B = 8  # on the instance: the class default stays off
    _, first, _ = runner.eval(x, normalize=dict(opt), **kw)
    ents = [e for e in runner._net_graphs.values() if e]
    assert len(ents) == 1 and torch.equal(first, want)
    keep = ents[0][4]
    assert keep and all(a is b for a, b in zip(keep, cg.norm_constants(norm_params(opt), 2, 70, 90, x.device)))
    before = [t.clone() for t in keep]
    for k in range(cg._CONST_CACHE_MAX + 6):
        cg.norm_constants(NormParams(tile_blocksize=32), 2, 100 + k, 90, x.device)
        cg.norm_constants(NormParams(lowhigh=(0.0, 10.0 + k)), 2, 70, 90, x.device)
    junk = [torch.full((8,), 1 << 20, dtype=torch.int32, device=gpu) for _ in range(256)]  # takes any freed small block
    assert not any(a is b for a, b in zip(keep, cg.norm_constants(norm_params(opt), 2, 70, 90, x.device)))  # evicted, rebuilt
    assert all(torch.equal(a, b) for a, b in zip(keep, before))  # the graph's own are untouched
    _, again, again_s = runner.eval(x, normalize=dict(opt), **kw)
    assert len([e for e in runner._net_graphs.values() if e]) == 1  # replayed, not captured anew
    assert torch.equal(again, want) and torch.equal(again_s, want_s)
    del junk

