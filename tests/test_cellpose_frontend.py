"""Cellpose front end on raw pixels: percentile select on uint8 / uint16 / float32 rows and the
normalising tile gather (``be_tiles_gather_norm``) against the sequence they replace,
``plan.gather(normalize99(x.float()), cpad)``, on the same device.  Every comparison of tiles is
``torch.equal`` on the bf16 bits."""
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


def _reference(plan, x, cpad, c_use, lower=1.0, upper=99.0):
    from bioengine_worker_amd.cellpose.gpu import normalize99

    return plan.gather(normalize99(x.float()[:, :c_use], lower, upper), cpad)


GEOMETRIES = {
    # several tiles per axis, both pads non-zero, overlapping tiles; rows of 6300 px, so odd rows
    # of uint16 and uint8 are not 16-byte aligned (scalar path) and even rows are
    "multi": dict(shape=(3, 2, 70, 90), bsize=32, c_use=2),
    # n = 1551: one chunk with a vector body and a tail for every type; C_use < cpad
    "odd": dict(shape=(1, 1, 33, 47), bsize=32, c_use=1),
    # the real tile size
    "tile224": dict(shape=(1, 2, 250, 230), bsize=224, c_use=2),
    # a third channel that must be ignored
    "wide": dict(shape=(2, 3, 70, 90), bsize=32, c_use=2),
}


@pytest.mark.parametrize("kind", ["uint8", "uint16", "float32"])
@pytest.mark.parametrize("geo", list(GEOMETRIES))
def test_gather_normalized_matches_normalize_then_gather(gpu, geo, kind):
    from bioengine_worker_amd.cellpose.gpu import TilePlan

    cfg = GEOMETRIES[geo]
    B, C, H, W = cfg["shape"]
    plan = TilePlan(H, W, cfg["bsize"], 0.1, device=gpu)
    if geo == "multi":
        assert len(plan.ys) > 1 and len(plan.xs) > 1 and plan.pad_y > 0 and plan.pad_x > 0
        assert plan.ys[1] - plan.ys[0] < plan.by  # overlapping tiles
    x = _data(cfg["shape"], kind).to(gpu)
    want = _reference(plan, x, 8, cfg["c_use"])
    got = plan.gather_normalized(x, 8, cfg["c_use"])
    assert got.shape == (B * plan.nt, plan.by, plan.bx, 8) and got.dtype == torch.bfloat16
    assert torch.equal(_bits(got), _bits(want))
    assert not got[..., cfg["c_use"]:].any()  # channel padding (and the ignored channel) is zero
    # cpad of two 8-channel groups: the second group is all padding
    assert torch.equal(_bits(plan.gather_normalized(x, 16, cfg["c_use"])), _bits(_reference(plan, x, 16, cfg["c_use"])))


@pytest.mark.parametrize("geo", list(GEOMETRIES))
def test_plain_gather_keeps_its_output(gpu, geo):
    """The un-normalised gather (new indexing) against a torch formulation of the same tiling."""
    from bioengine_worker_amd.cellpose.gpu import TilePlan

    cfg = GEOMETRIES[geo]
    B, C, H, W = cfg["shape"]
    plan = TilePlan(H, W, cfg["bsize"], 0.1, device=gpu)
    x = _data(cfg["shape"], "float32").to(gpu)
    xp = torch.zeros(B, 8, plan.Hp, plan.Wp, device=gpu)
    xp[:, :C, plan.pad_y: plan.pad_y + H, plan.pad_x: plan.pad_x + W] = x
    want = torch.stack([xp[b, :, y: y + plan.by, x0: x0 + plan.bx] for b in range(B) for y in plan.ys for x0 in plan.xs])
    want = want.permute(0, 2, 3, 1).to(torch.bfloat16)
    assert torch.equal(_bits(plan.gather(x, 8)), _bits(want))


def _rule_rows(kind):
    """[1, C, 70, 90] whose channels each exercise one rule of the normalisation."""
    g = torch.Generator().manual_seed(3)
    shape = (70, 90)
    if kind == "float32":
        rows = [torch.full(shape, 7.0),  # constant: all zeros
                5.0 + torch.rand(shape, generator=g) * 1e-4,  # p99 - p1 <= 1e-3: scale 1
                torch.randn(shape, generator=g) * 100,
                torch.rand(shape, generator=g) * 1e-3 - 5e-4]  # straddles zero, keys of both signs
        return torch.stack(rows)[None]
    two = torch.where(torch.rand(shape, generator=g) < 0.3, 1000, 1003)  # ties across all six ranks
    span = torch.randint(0, 65536, shape, generator=g)
    span[0, 0], span[0, 1] = 0, 65535
    low = 0x1200 + torch.randint(0, 256, shape, generator=g)  # values differ only in the low byte
    one_low = torch.where(torch.rand(shape, generator=g) < 0.995, 0x1200, 0x12ff)  # both percentiles on one value
    rows = [torch.full(shape, 4660), two, span, low, one_low]
    x = torch.stack(rows)[None].to(torch.int32)
    if kind == "uint8":
        x = x & 255
        return x.to(torch.uint8)
    return x.to(torch.uint16)


@pytest.mark.parametrize("pct", [(1.0, 99.0), (0.5, 99.5)])
@pytest.mark.parametrize("kind", ["uint8", "uint16", "float32"])
def test_rows_that_exercise_the_rules(gpu, kind, pct):
    from bioengine_worker_amd.cellpose.gpu import TilePlan

    x = _rule_rows(kind).to(gpu)
    C = x.shape[1]
    plan = TilePlan(70, 90, 32, 0.1, device=gpu)
    want = _reference(plan, x, 8, C, *pct)
    got = plan.gather_normalized(x, 8, C, *pct)
    assert torch.equal(_bits(got), _bits(want))
    assert not got[..., 0].any()  # the constant channel
    assert got[..., 1].any()
    if kind == "float32":
        # scale 1: the narrow channel comes out as x - p1, far below 1 in magnitude
        assert 0 < float(got[..., 1].float().abs().max()) < 1e-3


def test_workspace_reuse_and_shared_row_counts(gpu):
    from bioengine_worker_amd.cellpose import gpu as cg

    plan = cg.TilePlan(70, 90, 32, 0.1, device=gpu)
    a = _data((3, 2, 70, 90), "uint16", seed=1).to(gpu)
    b = _data((1, 1, 70, 90), "uint16", seed=2).to(gpu)

    def fresh(x):
        cg._pct_ws.clear()
        return plan.gather_normalized(x, 8)

    fa, fb = fresh(a), fresh(b)
    cg._pct_ws.clear()
    outs = [plan.gather_normalized(x, 8) for x in (a, a, b, a, b)]
    assert len(cg._pct_ws) == 1  # one workspace served all five calls
    for got, want in zip(outs, (fa, fa, fb, fa, fb)):
        assert torch.equal(_bits(got), _bits(want))
    # and the fp32 entry point shares it too
    assert torch.equal(_bits(plan.gather(cg.normalize99(a.float()), 8)), _bits(fa))
    assert torch.equal(_bits(plan.gather_normalized(b, 8)), _bits(fb))


@pytest.mark.parametrize("shape,kind", [((3, 2, 37, 53), "float"), ((4, 2, 128, 128), "uint16"),
                                        ((2, 1, 64, 64), "const"), ((32, 2, 512, 512), "uint16"),
                                        ((2, 3, 100, 101), "neg")])
def test_normalize99_keeps_its_results(gpu, shape, kind):
    """``normalize99`` (fp32 path, now with 16-byte loads) against the sort formulation under the
    tolerance of ``test_normalize99_radix_select_matches_sort_and_numpy``, and the same data at a
    16-byte aligned base (vector loads) against a base one element off (scalar loads): equal bits."""
    from bioengine_worker_amd.cellpose.gpu import normalize99, normalize99_sort

    g = torch.Generator().manual_seed(0)
    if kind == "uint16":
        x = (torch.rand(shape, generator=g) ** 4 * 4000).round()
    elif kind == "const":
        x = torch.full(shape, 7.0)
        x[1] = torch.rand(shape[1:], generator=g)
    elif kind == "neg":
        x = torch.randn(shape, generator=g) * 100
    else:
        x = torch.rand(shape, generator=g)
    xd = x.to(gpu)
    a = normalize99(xd)
    torch.testing.assert_close(a, normalize99_sort(xd), rtol=0, atol=1e-6)
    n = xd.numel()
    off = torch.empty(n + 1, device=gpu)[1:].view(shape)
    off.copy_(xd)
    assert off.is_contiguous() and off.data_ptr() != xd.data_ptr()
    assert torch.equal(normalize99(off), a)


def _spy_calls(monkeypatch):
    from bioengine_worker_amd.ops import _native

    names = []
    real = _native.call

    def call(name, *args):
        names.append(name)
        return real(name, *args)

    monkeypatch.setattr(_native, "call", call)
    return names


@pytest.fixture(scope="module")
def runner(gpu):
    from bioengine_worker_amd.cellpose.pipeline import CellposeRunner

    return CellposeRunner(device=gpu, seed=0)


@pytest.fixture(scope="module")
def cells(gpu):
    from bioengine_worker_amd.cellpose.pipeline import synthetic_cells

    a = synthetic_cells(2, 96, 128, ncells=12)
    return torch.from_numpy(a).to(gpu), torch.from_numpy(np.ascontiguousarray(a[::-1])).to(gpu)


def _eval_arm(monkeypatch, runner, fused, fn):
    from bioengine_worker_amd.cellpose import gpu as cg

    monkeypatch.setattr(cg, "FUSED_FRONT", fused)
    names = _spy_calls(monkeypatch)
    out = fn()
    torch.cuda.synchronize()
    assert ("be_tiles_gather_norm" in names) == fused
    assert ("be_pct_normalize" in names) != fused
    return out


def test_eval_same_with_switch_on_and_off(gpu, runner, cells, monkeypatch):
    on = _eval_arm(monkeypatch, runner, True, lambda: runner.eval(cells[0]))
    off = _eval_arm(monkeypatch, runner, False, lambda: runner.eval(cells[0]))
    for a, b in zip(on, off):
        assert torch.equal(a, b)
    assert on[0].shape == (2, 96, 128) and torch.isfinite(on[1]).all()


def test_stream_same_with_switch_on_and_off(gpu, runner, cells, monkeypatch):
    def three():
        st = runner.stream()
        outs = [st.submit(cells[0]), st.submit(cells[1]), st.submit(cells[0])]
        assert outs[0] is None
        return outs[1:] + [st.flush()]

    on = _eval_arm(monkeypatch, runner, True, three)
    off = _eval_arm(monkeypatch, runner, False, three)
    for r_on, r_off in zip(on, off):
        for a, b in zip(r_on, r_off):
            assert torch.equal(a, b)


def test_other_inputs_take_the_float_sequence(gpu, runner, cells, monkeypatch):
    """int32 pixels and a channel-last view are not read raw: they are converted and give what
    their float32 NCHW form (which the fused front end does read) gives."""
    names = _spy_calls(monkeypatch)
    xf = cells[0].float()
    want = runner.eval(xf)
    assert "be_tiles_gather_norm" in names
    for x in (cells[0].to(torch.int32), xf.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)):
        del names[:]
        assert x.dtype == torch.int32 or not x.is_contiguous()
        got = runner.eval(x)
        assert "be_tiles_gather_norm" not in names and "be_pct_normalize" in names
        for a, b in zip(got, want):
            assert torch.equal(a, b)


def test_error_codes_launch_nothing(gpu):
    from bioengine_worker_amd.cellpose import gpu as cg
    from bioengine_worker_amd.ops import _native

    plan = cg.TilePlan(70, 90, 32, 0.1, device=gpu)
    x = _data((1, 2, 70, 90), "uint16").to(gpu)
    ws = torch.zeros(64 * 6 * 258 * 4, dtype=torch.uint8, device=gpu)
    fn = _native.hip().be_tiles_gather_norm

    def rc(dtype=1, B=1, cpad=8):
        out = torch.full((plan.nt, plan.by, plan.bx, 16), 1.0, dtype=torch.bfloat16, device=gpu)
        code = fn(_native.ptr(x), dtype, B, 2, 2, 70, 90, 1.0, 99.0, plan.pad_y, plan.pad_x, _native.ptr(plan.ys_t),
                  _native.ptr(plan.xs_t), len(plan.ys), len(plan.xs), plan.by, plan.bx, cpad, _native.ptr(out),
                  _native.ptr(ws), ws.numel(), _native.stream(gpu))
        torch.cuda.synchronize()
        untouched = bool((out == 1.0).all()) and not bool(ws.any())
        return code, untouched

    assert rc() == (0, False)  # the valid call writes tiles and leaves its state in the workspace
    ws.zero_()
    for bad in (dict(cpad=12), dict(B=40000), dict(dtype=7), dict(dtype=-1)):
        code, untouched = rc(**bad)
        assert code != 0 and untouched, bad
