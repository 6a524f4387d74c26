"""Integer data for the per-layer fused conv kernel (``csrc/kernels/conv2d_nhwc.hip``), for which the
right answer does not depend on the order of summation, and an independent float64 model of the
operation.  Tests compare with ``torch.equal``.

Why equality is legitimate.  Inputs are integers (x in [-3, 3], x2 in [-2, 2]), scales are 0.5, 1 or 2,
shifts integers in [-2, 2]: every activated value is a multiple of 0.5 of magnitude <= 12, hence a bf16
number.  Weights are integers in [-2, 2] (kept with probability ``dens``), bias in [-4, 4], residual
in [-8, 8].  Every product and every partial sum is then a multiple of 0.5 below 2^22, exact in fp32 in
any order -- whatever order the MFMA uses inside.  The one rounding left is the fp32 -> bf16 store,
whose result round-to-nearest-even fixes.  :func:`check_exactness` asserts these preconditions on the
float64 model alone.

What rounds.  bf16 keeps 8 significant bits, so an output rounds only if it has a half above 128 or is
odd above 256.  The spread of an output grows as ``sqrt(K * dens)``, K = ``ks * ks * cin``: at ``dens``
= 1 the 3x3 layers of 128 and 256 input channels reach |y| of 400 .. 660 and round 13 % .. 19 % of
their outputs, those of 32 and 64 channels a few per cent, and no 1x1 layer of the list and no
one-pixel image gets above 128 at all.  Cases built to round carry ``rounds=True`` and must have
between 5 % and 95 % of their outputs rounded and at least 100 distinct values.  The others cannot
meet that under these draws whatever ``dens`` is (a 1 x 1 image of 32 channels has 96 outputs): their
outputs are mostly or wholly representable, they pin indexing (taps, pixels, channels, images,
padding), and they must hold ``min(100, numel / 4)`` distinct values.  ``test_conv_exact.py`` asserts
that the rounding cases reach every store path of the kernel.

``ref64`` shares no code with ``ops/conv.py``: index arithmetic for the up-sampling and the pool, the
activation written out, explicit zero padding after it, ``F.conv2d`` in float64 on the raw
``[cout, cin, ks, ks]`` weight.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from types import SimpleNamespace

import torch
import torch.nn.functional as F

TW = 32  # the kernel's tile is 2 * nw rows x 32 columns


@dataclass(frozen=True)
class Case:
    name: str
    ks: int = 3
    cin: int = 32
    cout: int = 32
    H: int = 13
    W: int = 45
    N: int = 3
    inmode: str = "none"          # none | up2 | pool2
    odd_src: bool = False         # pool2 from a (2H + 1, 2W + 1) source
    scale: str | None = "shared"  # None | shared [C] | rows [N, C] | strided (columns C..2C of [N, 3C])
    shift: str | None = "rows"
    x2: bool = False
    res: bool = False
    out: str | None = None        # None | given (out=) | alias (out is the residual)
    post: str | None = None       # None | shared | rows | strided | scale (no shift) | shift (no scale)
    relu: bool = True
    post_relu: bool = False
    no_bias: bool = False
    bias: bool = True
    head: bool = False            # f32 NCHW head, cout_valid = cout, cout_pad_to = 16
    exact_cin: bool = False
    nw: int | None = None
    persist: int = 0
    dens: float = 1.0
    rounds: bool = False
    seed: int = 0
    # expected kernel template, asserted against PackedConv.choose: (ck, tco)
    tmpl: tuple | None = None

    @property
    def src_hw(self):
        if self.inmode == "up2":
            return self.H // 2, self.W // 2
        if self.inmode == "pool2":
            return 2 * self.H + int(self.odd_src), 2 * self.W + int(self.odd_src)
        return self.H, self.W


def _ri(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _affine(g, kind, N, C, draw):
    """-> (tensor as the op takes it, the wide parent or None).  ``strided``: a column slice, row stride
    3 C, offset C (16-byte aligned as C % 4 == 0)."""
    if kind is None:
        return None
    if kind == "shared":
        return draw(C)
    if kind == "rows":
        return draw(N, C)
    assert kind == "strided"
    return draw(N, 3 * C)[:, C:2 * C]


def packed(case: Case, w, bias):
    from bioengine_worker_amd.ops.conv import PackedConv

    pc = PackedConv.from_weight(w, bias, cout_pad_to=16 if case.head else None, exact_cin=case.exact_cin)
    if case.tmpl is not None:
        assert (pc.ck, pc.tco) == case.tmpl, (case.name, pc.ck, pc.tco)
    return pc


def make(case: Case) -> SimpleNamespace:
    """The seeded draws of one case, as CPU tensors in the layout the op takes."""
    g = torch.Generator().manual_seed(1000 + case.seed)
    N, H, W = case.N, case.H, case.W
    Hs, Ws = case.src_hw
    w = _ri(g, -2, 2, case.cout, case.cin, case.ks, case.ks)
    w = w * (torch.rand(w.shape, generator=g) < case.dens)
    nz = _ri(g, 1, 2, case.cout, 2, case.ks, case.ks) * (2 * _ri(g, 0, 1, case.cout, 2, case.ks, case.ks) - 1)
    w[:, :2] = nz  # channels 0 and 1 carry the border-visible shifts below: their weights are never zero
    bias = _ri(g, -4, 4, case.cout) if case.bias else None
    pc = packed(case, w, bias)
    C = pc.cin_pad
    d = SimpleNamespace(case=case, w=w, bias=bias, pc=pc, C=C)
    d.x = _ri(g, -3, 3, N, Hs, Ws, C).bfloat16()
    d.x2 = _ri(g, -2, 2, N, H, W, C).bfloat16() if case.x2 else None
    d.scale = _affine(g, case.scale, N, C, lambda *s: 2.0 ** _ri(g, -1, 1, *s))
    d.shift = _affine(g, case.shift, N, C, lambda *s: _ri(g, -2, 2, *s))
    if d.shift is not None:
        # act(0) = relu?(shift) != 0 in every image: padding applied before the activation is visible
        # along every border.  Without the ReLU channel 1 keeps a negative activation of zero.
        d.shift[..., 0] = 2.0
        d.shift[..., 1] = 1.0 if case.relu else -1.0
    d.res = _ri(g, -8, 8, N, H, W, case.cout).bfloat16() if case.res else None
    qs = qt = None
    if case.post is not None:
        kind = {"scale": "shared", "shift": "shared"}.get(case.post, case.post)
        if case.post != "shift":
            qs = 2.0 ** _ri(g, -1, 1, case.cout)
        if case.post != "scale":
            qt = _affine(g, kind, N, case.cout, lambda *s: _ri(g, -4, 4, *s))
    d.post_scale, d.post_shift = qs, qt
    return d


def _rows(t, N):
    """[C] or [N, C] affine -> float64 broadcastable over NHWC."""
    t = t.double()
    return t[:, None, None, :] if t.dim() == 2 else t


def activated(d, shift=None) -> torch.Tensor:
    """[N, H, W, cin] float64: inxform, + x2, * scale, + shift, ReLU -- by index, no library pooling."""
    c = d.case
    x = d.x.double()
    iy, ix = torch.arange(c.H), torch.arange(c.W)
    if c.inmode == "up2":
        x = x[:, iy // 2][:, :, ix // 2]
    elif c.inmode == "pool2":  # floor: an odd source loses its last row / column
        q = [x[:, 2 * iy + dy][:, :, 2 * ix + dx] for dy in (0, 1) for dx in (0, 1)]
        x = torch.maximum(torch.maximum(q[0], q[1]), torch.maximum(q[2], q[3]))
    if d.x2 is not None:
        x = x + d.x2.double()
    if d.scale is not None:
        x = x * _rows(d.scale, c.N)
    shift = d.shift if shift is None else shift
    if shift is not None:
        x = x + _rows(shift, c.N)
    if c.relu:
        x = x.clamp_min(0.0)
    return x[..., : c.cin]


def padded(a: torch.Tensor, ks: int) -> torch.Tensor:
    """Zero padding AFTER the activation: [N, H + ks - 1, W + ks - 1, cin]."""
    p = ks // 2
    N, H, W, C = a.shape
    ap = torch.zeros(N, H + 2 * p, W + 2 * p, C, dtype=a.dtype)
    ap[:, p:p + H, p:p + W] = a
    return ap


def conv64(ap: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """The bare sum over taps and channels of a padded NHWC image, float64, NHWC."""
    return F.conv2d(ap.permute(0, 3, 1, 2), w.double()).permute(0, 2, 3, 1).contiguous()


def rne(y: torch.Tensor) -> torch.Tensor:
    """One round-to-nearest-even cast to bf16 (the values are fp32 numbers, so float64 -> bf16 rounds once)."""
    return y.to(torch.bfloat16)


def epilogue(y: torch.Tensor, d, res=None, cast=rne) -> torch.Tensor:
    """``y``: the bare conv sum.  + bias, + residual, then the f32 head (float64 NCHW, itself the answer)
    or one bf16 cast; on the post-affine path ``bf16(y) * qs + qt``, ReLU, a second cast."""
    c = d.case
    if d.bias is not None and not c.no_bias:
        y = y + d.bias.double()
    if c.head:
        y = y.permute(0, 3, 1, 2).contiguous()
        return y.clamp_min(0.0) if c.post_relu else y
    res = d.res if res is None else res
    if res is not None:
        y = y + res.double()
    if d.post_scale is None and d.post_shift is None:
        return cast(y.clamp_min(0.0) if c.post_relu else y)
    v = cast(y).double()
    if d.post_scale is not None:
        v = v * d.post_scale.double()
    if d.post_shift is not None:
        v = v + _rows(d.post_shift, c.N)
    return cast(v.clamp_min(0.0) if c.post_relu else v)


def presum(d) -> torch.Tensor:
    """The exact float64 value in front of the (first) cast, NHWC; the head's value without its ReLU."""
    c = d.case
    y = conv64(padded(activated(d), c.ks), d.w)
    if d.bias is not None and not c.no_bias:
        y = y + d.bias.double()
    if d.res is not None and not c.head:
        y = y + d.res.double()
    return y


def ref64(d) -> torch.Tensor:
    """*The* answer: bf16 NHWC, or float64 NCHW for the head."""
    return epilogue(conv64(padded(activated(d), d.case.ks), d.w), d)


def check_exactness(d) -> dict:
    """The conditions on the inputs under which equality may be demanded, checked on the model alone."""
    c = d.case
    a = activated(d)
    assert torch.equal(a, a.to(torch.bfloat16).double()), f"{c.name}: an activated value is no bf16 number"
    for t in (d.w, d.bias, d.res, d.post_scale, d.post_shift):
        assert t is None or torch.equal(t.double(), t.to(torch.bfloat16).double())
    mag = conv64(padded(a.abs(), c.ks), d.w.abs())
    if d.bias is not None:
        mag = mag + d.bias.abs().double()
    if d.res is not None:
        mag = mag + d.res.abs().double()
    assert mag.max().item() < 2 ** 22, f"{c.name}: a partial sum may leave the exact range of fp32"
    y = presum(d)
    assert torch.equal(y * 2, (y * 2).round()), f"{c.name}: an output is no multiple of 0.5"
    out = ref64(d)
    distinct = out.unique().numel()
    if c.head:
        frac = 0.0
    elif d.post_scale is None and d.post_shift is None:
        frac = (rne(y).double() != y).double().mean().item()
    else:  # either cast may round
        v = rne(y).double() * (1.0 if d.post_scale is None else d.post_scale.double())
        v = v + (0.0 if d.post_shift is None else _rows(d.post_shift, c.N))
        frac = ((rne(y).double() != y) | (rne(v).double() != v)).double().mean().item()
    if c.rounds:
        assert 0.05 <= frac <= 0.95, f"{c.name}: {frac:.3f} of the outputs round (want 5 % .. 95 %)"
        assert distinct >= 100, f"{c.name}: {distinct} distinct outputs"
    else:
        assert distinct >= min(100, out.numel() // 4), f"{c.name}: {distinct} distinct outputs of {out.numel()}"
    return dict(frac=frac, distinct=distinct, maxabs=y.abs().max().item())


def tile_rows(d, nw=None) -> int:
    """Rows of the kernel's pixel tile for this case: 2 * nw."""
    from bioengine_worker_amd.ops.conv import choose_nw

    c = d.case
    return 2 * int(nw or c.nw or choose_nw(d.pc, c.H, c.W, c.inmode, d.x2 is not None))


def assert_exact(got: torch.Tensor, want: torch.Tensor, name: str, th: int = 8, nchw: bool = False, tco: int = 64):
    """``torch.equal`` with a report that points at the tile: count, first (n, y, x, co), expected and got,
    tile (y // th, x // 32), position in the tile, output-channel block."""
    assert got.shape == want.shape, f"{name}: shape {tuple(got.shape)} != {tuple(want.shape)}"
    if nchw:
        got, want = got.permute(0, 2, 3, 1), want.permute(0, 2, 3, 1)
    g, w = got.double().cpu(), want.double().cpu()
    g, w = g.reshape(-1, *g.shape[-3:]), w.reshape(-1, *w.shape[-3:])  # a volume's slices count as images
    bad = g != w
    if not bad.any():
        return
    idx = bad.nonzero()
    first = tuple(idx[0].tolist())
    n, y, x, co = first
    tiles = sorted({(int(i[1]) // th, int(i[2]) // TW) for i in idx[:2000]})
    raise AssertionError(
        f"{name}: {int(bad.sum())} of {bad.numel()} outputs differ; first at (n, y, x, co) = {first}: expected "
        f"{w[first].item()}, got {g[first].item()}; tile (y // {th}, x // {TW}) = ({y // th}, {x // TW}), in-tile "
        f"({y % th}, {x % TW}), channel block {co // tco} (+{co % tco}); tiles hit: {tiles[:12]}")


# ------------------------------------------------------------------------------------------- mutants
# Faults of the kind a kernel can have, injected into the float64 model.  Each returns the mutated
# answer, or None where the case does not offer the fault (no border, no residual, ...).


def trunc(y: torch.Tensor) -> torch.Tensor:
    """fp32 -> bf16 toward zero."""
    return (y.float().view(torch.int32) & ~0xFFFF).view(torch.float32).to(torch.bfloat16)


def mut_truncate(d, th):
    return epilogue(conv64(padded(activated(d), d.case.ks), d.w), d, cast=trunc)


def mut_corner_act0(d, th):
    """One out-of-image corner halo pixel holds act(0): padding applied before the activation there."""
    c = d.case
    if c.ks != 3 or d.shift is None:
        return None
    ap = padded(activated(d), 3)
    zero = SimpleNamespace(**vars(d))
    zero.x = torch.zeros_like(d.x)
    zero.x2 = None if d.x2 is None else torch.zeros_like(d.x2)
    n = c.N - 1
    ap[n, c.H + 1, c.W + 1] = activated(zero)[n, 0, 0]
    return epilogue(conv64(ap, d.w), d)


def mut_drop_product(d, th):
    """One (pixel, tap, channel) product missing from one output."""
    c = d.case
    ap = padded(activated(d), c.ks)
    y = conv64(ap, d.w)
    n, yy, xx = c.N - 1, c.H // 2, c.W // 2
    prod = ap[n, yy:yy + c.ks, xx:xx + c.ks, :].permute(2, 0, 1)[None] * d.w.double()  # [co, ci, ty, tx]
    hit = prod.nonzero()
    if not len(hit):
        return None
    co, ci, ty, tx = hit[len(hit) // 2].tolist()
    y[n, yy, xx, co] -= prod[co, ci, ty, tx]
    return epilogue(y, d)


def mut_shift_of_image0(d, th):
    """Image 1's shift taken from image 0 inside one th x 32 tile (a stale affine prefetch)."""
    c = d.case
    if d.shift is None or d.shift.dim() != 2 or c.N < 2:
        return None
    sh = d.shift.clone()
    sh[1] = d.shift[0]
    y = conv64(padded(activated(d), c.ks), d.w)
    yalt = conv64(padded(activated(d, shift=sh), c.ks), d.w)
    y[1, :th, :TW] = yalt[1, :th, :TW]
    return epilogue(y, d)


def mut_zero_channel_group(d, th):
    """Channels 8..15 of one in-image halo pixel are zero for the tile that reads it as halo."""
    c = d.case
    if c.ks != 3 or c.cin < 16 or c.H <= th:
        return None
    a = activated(d)
    y = conv64(padded(a, 3), d.w)
    a[0, th, 5, 8:16] = 0  # first row below tile (0, 0)
    yalt = conv64(padded(a, 3), d.w)
    y[0, :th, :TW] = yalt[0, :th, :TW]
    return epilogue(y, d)


def mut_residual_next_column(d, th):
    """The last column of a tile adds the residual of the pixel to its right."""
    c = d.case
    if d.res is None or c.head or c.W <= TW:
        return None
    res = d.res.clone()
    res[:, :th, TW - 1] = d.res[:, :th, TW]
    return epilogue(conv64(padded(activated(d), c.ks), d.w), d, res=res)


MUTANTS = {
    "truncate": mut_truncate,
    "corner_act0": mut_corner_act0,
    "drop_product": mut_drop_product,
    "shift_of_image0": mut_shift_of_image0,
    "zero_channel_group": mut_zero_channel_group,
    "residual_next_column": mut_residual_next_column,
}


# --------------------------------------------------------------------------------------------- cases


def _grid_cases():
    """The template grid: every (ks, ck, tco) the entry point dispatches, both nw, every INMODE, X2."""
    out = []
    #        cin, exact, ck
    chans = [(8, False, 8), (16, True, 8), (24, True, 8), (32, False, 32), (64, False, 32)]
    couts = [(16, 16), (32, 32), (64, 64)]
    i = 0
    for ks in (3, 1):
        for cin, exact, ck in chans:
            ckk = 64 if (ks == 1 and cin == 64) else ck
            for cout, tco in couts:
                # rotate nw, INMODE and the affine forms through the grid; the dedicated groups below
                # cross them on purpose
                nw = (4, 8)[i % 2]
                inmode = ("none", "up2", "pool2")[(i // 2) % 3]
                H, W = {"none": (13, 45), "up2": (18, 34), "pool2": (9, 33)}[inmode]
                out.append(Case(f"grid_ks{ks}_cin{cin}_ck{ckk}_tco{tco}_nw{nw}_{inmode}", ks=ks, cin=cin, cout=cout,
                                H=H, W=W, inmode=inmode, exact_cin=exact, nw=nw, tmpl=(ckk, tco), seed=i,
                                relu=i % 3 != 2))
                i += 1
    # both nw x every INMODE on both kernels (persistent tco 32, one-block tco 64), and X2 on INMODE none
    for tco, cin, cout in ((32, 32, 32), (64, 32, 64)):
        for nw in (4, 8):
            for inmode, (H, W) in (("none", (17, 65)), ("up2", (18, 34)), ("pool2", (9, 33))):
                out.append(Case(f"mode_tco{tco}_nw{nw}_{inmode}", cin=cin, cout=cout, H=H, W=W, inmode=inmode, nw=nw,
                                tmpl=(32, tco), seed=100 + len(out)))
            out.append(Case(f"x2_tco{tco}_nw{nw}", cin=cin, cout=cout, H=17, W=65, x2=True, nw=nw, tmpl=(32, tco),
                            seed=100 + len(out)))
    out.append(Case("x2_ck8_tco16_1x1", ks=1, cin=8, cout=16, H=9, W=32, x2=True, tmpl=(8, 16), seed=131))
    out.append(Case("x2_ck64_tco64_1x1", ks=1, cin=64, cout=64, H=9, W=32, x2=True, tmpl=(64, 64), seed=132))
    out.append(Case("cin20_padded_to_32_input_garbage_beyond", cin=20, cout=32, tmpl=(32, 32), seed=133))
    return out


def _cout_cases():
    r = dict(cin=128, rounds=True)  # K = 1152: these round, so every store path sees ties and halves
    return [
        Case("cout12_unstaged_tco16", cout=12, x2=True, res=True, tmpl=(32, 16), seed=200, **r),
        Case("cout20_unstaged_tco32", cout=20, x2=True, res=True, tmpl=(32, 32), seed=201, **r),
        Case("cout12_unstaged_tco16_nw4_1x1", ks=1, cin=8, cout=12, nw=4, tmpl=(8, 16), seed=202),
        Case("cout24_staged_partial_block", cout=24, x2=True, res=True, tmpl=(32, 32), seed=203, **r),
        Case("cout48_staged_partial_block_tco64", cout=48, x2=True, res=True, tmpl=(32, 64), seed=204, **r),
        Case("cout68_unstaged_tco64", cout=68, x2=True, res=True, tmpl=(32, 64), seed=205, **r),
        Case("cout96_tco64_second_block_half_empty", cout=96, x2=True, res=True, tmpl=(32, 64), seed=206, **r),
        # order-2 XCD remap with a block count that is no multiple of 8: (17, 65) at nw 4 is 3 images x
        # 3 x 3 tiles x 4 channel blocks = 108 blocks
        Case("cout256_four_blocks_xcd_remap_108_blocks", cin=32, cout=256, H=17, W=65, nw=4, tmpl=(32, 64), seed=207),
        Case("cout256_cin256_rounds", cin=256, cout=256, H=8, W=32, N=2, res=True, rounds=True, tmpl=(32, 64), seed=208),
    ]


def _geometry_cases():
    out = []
    sizes = [(1, 1), (1, 33), (2, 31), (9, 32), (17, 65), (8, 64), (16, 32), (13, 45)]
    for i, (H, W) in enumerate(sizes):
        for tco, cout in ((32, 32), (64, 64)):
            nw = (4, 8)[(i + tco // 64) % 2] if (H, W) not in ((8, 64), (16, 32)) else (4 if H == 8 else 8)
            out.append(Case(f"geom_{H}x{W}_tco{tco}_nw{nw}", cin=32, cout=cout, H=H, W=W, nw=nw, res=True,
                            seed=300 + len(out)))
    out += [
        Case("pool2_odd_source_tco32", cin=32, cout=32, H=9, W=33, inmode="pool2", odd_src=True, seed=320),
        Case("pool2_odd_source_tco64_ck8", cin=8, cout=64, H=5, W=17, inmode="pool2", odd_src=True, seed=321),
        Case("up2_to_2x2", cin=32, cout=32, H=2, W=2, inmode="up2", seed=322),
        Case("up2_to_34x66_tco32", cin=32, cout=32, H=34, W=66, inmode="up2", seed=323),
        Case("up2_to_34x66_tco64", cin=64, cout=64, H=34, W=66, inmode="up2", seed=324),
    ]
    return out


def _affine_cases():
    out = []
    forms = [("rows", "shared"), ("shared", "rows"), ("rows", "rows"), ("strided", "shared"), ("shared", "strided"),
             ("strided", "strided"), ("shared", "shared"), (None, "rows"), ("rows", None), (None, None)]
    for i, (sc, sh) in enumerate(forms):
        for tco, cout in ((32, 32), (64, 64))[: 2 if i % 2 == 0 else 1]:  # the one-block kernel: every other form
            out.append(Case(f"affine_scale_{sc}_shift_{sh}_tco{tco}", cin=64, cout=cout, H=13, W=45, scale=sc, shift=sh,
                            relu=i % 2 == 0, seed=400 + len(out)))
    return out


def _persist_cases():
    out = []
    for blocks in (1, 3, 7):
        # (17, 65) at nw 8: 2 x 3 = 6 tiles per image, 18 in all (nw 4: 9 and 27).  3 and 7 blocks leave
        # ragged ranges, and a block's next tile (+3, +7) is often in the next image: its affine rows and
        # halo are prefetched across the image boundary
        out.append(Case(f"persist{blocks}_resident_weights", cin=32, cout=32, H=17, W=65, nw=8, persist=blocks,
                        scale="rows", shift="rows", res=True, seed=500 + blocks))
        for cin, cout in ((64, 16), (128, 32)):
            out.append(Case(f"persist{blocks}_nchunk{cin // 32}_cin{cin}_cout{cout}", cin=cin, cout=cout, H=17, W=65,
                            nw=(4, 8)[(blocks // 2) % 2], persist=blocks, scale="strided", shift="strided", x2=cin == 128,
                            res=True, rounds=cin == 128, seed=510 + blocks + cin))
    out.append(Case("persist3_up2_nchunk2", cin=64, cout=32, H=18, W=34, inmode="up2", persist=3, seed=530))
    out.append(Case("persist7_pool2_ck8_nchunk3", cin=24, exact_cin=True, cout=16, H=9, W=33, inmode="pool2", persist=7,
                    seed=531))
    return out


def _epilogue_cases():
    out = []
    base = dict(cin=128, H=13, W=45, x2=True, rounds=True)
    for tco, cout in ((32, 32), (64, 64)):
        b = dict(base, cout=cout)
        out += [
            Case(f"epi_residual_tco{tco}", res=True, seed=600 + tco, **b),
            Case(f"epi_out_aliases_residual_tco{tco}", res=True, out="alias", seed=602 + tco, **b),
            Case(f"epi_post_relu_tco{tco}", res=True, post_relu=True, seed=604 + tco, **b),
            Case(f"epi_post_affine_shared_relu_tco{tco}", post="shared", post_relu=True, seed=605 + tco, **b),
            Case(f"epi_post_affine_rows_relu_tco{tco}", post="rows", post_relu=True, res=True, seed=606 + tco, **b),
        ]
        if tco == 64:  # the epilogue is one function for both kernels: the rest once
            continue
        out += [
            Case(f"epi_out_given_tco{tco}", out="given", seed=601 + tco, **b),
            Case(f"epi_no_bias_tco{tco}", no_bias=True, seed=603 + tco, **b),
            Case(f"epi_post_affine_strided_tco{tco}", post="strided", seed=607 + tco, **b),
            Case(f"epi_post_scale_only_tco{tco}", post="scale", post_relu=True, seed=608 + tco, **b),
            Case(f"epi_post_shift_only_tco{tco}", post="shift", seed=609 + tco, **b),
        ]
    out.append(Case("epi_post_affine_unstaged_cout20", cout=20, post="rows", post_relu=True, res=True, seed=620, **base))
    for bias in (True, False):
        for pr in (False, True):
            out.append(Case(f"head_f32_nchw_cout3_bias{int(bias)}_relu{int(pr)}", ks=1, cin=32, cout=3, H=13, W=45,
                            head=True, bias=bias, post_relu=pr, relu=not pr, seed=630 + 2 * bias + pr))
    out.append(Case("head_f32_nchw_3x3_cin128", cin=128, cout=3, H=17, W=65, head=True, seed=640))
    return out


@functools.lru_cache(maxsize=None)
def cases() -> tuple:
    out = _grid_cases() + _cout_cases() + _geometry_cases() + _affine_cases() + _persist_cases() + _epilogue_cases()
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


def by_name(name: str) -> Case:
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def data(name: str) -> SimpleNamespace:
    """The case's draws and its answer (``d.want``), made once and shared; tests must not write to them."""
    d = make(by_name(name))
    d.want = ref64(d)
    return d


def run(d, device=None, nw=None, frag=False) -> torch.Tensor:
    """``fused_conv2d`` of the case on ``device`` (None: the CPU path on the bf16 tensors).  Without
    ``frag`` the conv has no fragment-order weights, so the entry point cannot pick a ping-pong build."""
    import copy

    from bioengine_worker_amd.ops import _native
    from bioengine_worker_amd.ops.conv import fused_conv2d

    c = d.case
    if device is None:
        mv = lambda t: t
    else:  # a strided affine stays a column slice of its wide parent on the device
        mv = lambda t: None if t is None else (
            t.to(device) if t.is_contiguous() else t._base.to(device)[:, t.shape[1]:2 * t.shape[1]])
    pc = d.pc if device is None else copy.copy(d.pc).to(device)  # the shared case keeps its CPU tensors
    if frag:
        pc.frag()
    else:
        assert pc.frag_built() is None, "the per-layer kernel is under test: no fragment-order weights"
    res = None if d.res is None else mv(d.res.clone())
    out = None
    if c.out == "alias":
        out = res
    elif c.out == "given":
        out = torch.full((c.N, c.H, c.W, c.cout), 77.0, dtype=torch.bfloat16, device=res.device if res is not None else device)
    kw = dict(x2=mv(d.x2), scale=mv(d.scale), shift=mv(d.shift), relu=c.relu, residual=res, inmode=c.inmode,
              post_relu=c.post_relu, out=out, no_bias=c.no_bias, post_scale=mv(d.post_scale), post_shift=mv(d.post_shift),
              nw=nw or c.nw)
    if c.head:
        kw.update(out_nchw_f32=True, cout_valid=c.cout)
    if device is not None:
        for t in (kw["scale"], kw["shift"], kw["post_shift"]):
            assert t is None or t.is_contiguous() == (t.dim() == 1 or t.stride(0) == t.shape[1])
    if device is None or not c.persist:
        y = fused_conv2d(mv(d.x), pc, **kw)
    else:
        _native.call("be_conv2d_set_persist", c.persist)
        try:
            y = fused_conv2d(mv(d.x), pc, **kw)
            torch.cuda.synchronize()
        finally:
            _native.call("be_conv2d_set_persist", 0)
    if out is not None:
        assert y is out
    return y.cpu()


# ----------------------------------------------------------------------------------------- tap map


def tap_code(cout: int, cin: int) -> torch.Tensor:
    """w[co, ci, ty, tx] = ((7 co + 3 ci + 3 ty + tx) % 17) - 8."""
    co, ci, ty, tx = torch.meshgrid(torch.arange(cout), torch.arange(cin), torch.arange(3), torch.arange(3), indexing="ij")
    return (((7 * co + 3 * ci + 3 * ty + tx) % 17) - 8).float()


#: (cin, exact_cin, cout, nw, ck, tco): the one-block kernel with 32-channel chunks, the persistent one with 8
TAP_CONFIGS = [(64, False, 96, 4, 32, 64), (16, True, 20, 8, 8, 32), (64, False, 32, 8, 32, 32)]
TAP_HW = (17, 65)


def tap_map(cin, exact, cout, nw, ck, tco):
    """One image per (position, input channel): a single 1 at (y, x, ci).  -> (x bf16, pc, expected bf16):
    the flipped 3x3 stamp of codes around (y, x) -- out[y - ty + 1, x - tx + 1, co] = w[co, ci, ty, tx] --
    and zero elsewhere, built by index without a convolution."""
    from bioengine_worker_amd.ops.conv import PackedConv

    H, W = TAP_HW
    th = 2 * nw
    pos = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (th - 1, 31), (th, 32), (th - 1, 32), (th, 31), (H - 1, W - 1)]
    chans = sorted({0, 7, 8, ck - 1, ck % cin, cin - 1})
    w = tap_code(cout, cin)
    pc = PackedConv.from_weight(w, None, exact_cin=exact)
    assert (pc.ck, pc.tco, pc.cin_pad) == (ck, tco, cin)
    items = [(p, ci) for p in pos[:8] for ci in chans]
    x = torch.zeros(len(items), H, W, cin)
    want = torch.zeros(len(items), H, W, cout)
    for n, ((y, xx), ci) in enumerate(items):
        x[n, y, xx, ci] = 1.0
        for ty in range(3):
            for tx in range(3):
                oy, ox = y - ty + 1, xx - tx + 1
                if 0 <= oy < H and 0 <= ox < W:
                    want[n, oy, ox] = w[:, ci, ty, tx]
    return x.bfloat16(), pc, want.bfloat16()


# --------------------------------------------------------------------------- concat and 3-D entries
# No pre-activation here: x in [-3, 3] in steps of 0.5 (so the wide layers round), weights in [-2, 2], bias
# in [-4, 4], optional output ReLU.

#: name -> (Ca, Cb, cout, H, W, d2s, nw, post_relu); (8, 8) keeps its 16 channels (8-channel chunks)
CONCAT_CASES = {
    "concat_8_8_ck8_tco16": (8, 8, 16, 13, 45, False, 8, False),
    "concat_32_32_tco32": (32, 32, 32, 17, 65, False, 4, True),
    "concat_24_40_seam_inside_a_chunk_tco64": (24, 40, 64, 13, 45, False, 4, False),
    "concat_64_32_three_chunks_cout20": (64, 32, 20, 9, 32, False, 8, True),
    "concat_d2s_8_8_ck8": (8, 8, 32, 14, 46, True, 4, True),
    "concat_d2s_32_32": (32, 32, 64, 18, 66, True, 8, False),
    "concat_d2s_24_40": (24, 40, 24, 2, 34, True, 4, False),
    "concat_d2s_64_32": (64, 32, 64, 10, 32, True, 4, True),
}


@functools.lru_cache(maxsize=None)
def concat_data(name: str) -> SimpleNamespace:
    from bioengine_worker_amd.ops.conv import PackedConv

    Ca, Cb, cout, H, W, d2s, nw, post_relu = CONCAT_CASES[name]
    g = torch.Generator().manual_seed(2000 + sorted(CONCAT_CASES).index(name))
    N = 3
    w = _ri(g, -2, 2, cout, Ca + Cb, 3, 3)
    bias = _ri(g, -4, 4, cout)
    pc = PackedConv.from_weight(w, bias, exact_cin=True)
    assert pc.cin_pad == Ca + Cb and pc.ck == (8 if (Ca + Cb) % 32 else 32)
    xa = (_ri(g, -6, 6, N, H, W, Ca) / 2).bfloat16()
    if d2s:  # [N, H/2, W/2, 4 Cb], channel (2 dy + dx) * Cb + c = channel c of pixel (2y + dy, 2x + dx)
        xb = (_ri(g, -6, 6, N, H // 2, W // 2, 4 * Cb) / 2).bfloat16()
        full = torch.zeros(N, H, W, Cb, dtype=torch.float64)
        for dy in (0, 1):
            for dx in (0, 1):
                full[:, dy::2, dx::2] = xb[..., (2 * dy + dx) * Cb:(2 * dy + dx + 1) * Cb].double()
    else:
        xb = (_ri(g, -6, 6, N, H, W, Cb) / 2).bfloat16()
        full = xb.double()
    a = torch.cat([xa.double(), full], -1)
    y = conv64(padded(a, 3), w) + bias.double()
    want = rne(y.clamp_min(0.0) if post_relu else y)
    assert conv64(padded(a.abs(), 3), w.abs()).max().item() + 4 < 2 ** 22
    return SimpleNamespace(xa=xa, xb=xb, pc=pc, want=want, d2s=d2s, nw=nw, post_relu=post_relu,
                           frac=(rne(y).double() != y).double().mean().item())


#: name -> (cin, cout, N, D, H, W, BE_CONV3D_CK16, expected z-tap ck, post_relu)
CONV3D_CASES = {
    "ztaps_ck8_cin8_D1": (8, 16, 2, 1, 9, 20, "1", 8, False),
    "ztaps_ck8_cin16_D2": (16, 32, 1, 2, 13, 20, "0", 8, True),
    "ztaps_ck16_cin16_D5": (16, 20, 1, 5, 17, 20, "1", 16, False),
    "ztaps_ck16_cin16_D2": (16, 16, 2, 2, 9, 33, "1", 16, True),
    "ztaps_ck32_cin32_D5": (32, 64, 1, 5, 13, 20, "1", 32, True),
    "ztaps_ck32_cin32_D1": (32, 32, 2, 1, 16, 20, "1", 32, False),
}
#: name -> (Ca, Cb, cout, N, D, H, W, BE_CONV3D_CK16, expected ck); the concat build has 8- and 32-channel
#: chunks only, so a 16-channel concatenation fuses only with 8-channel chunks (``concat3d_fusible``)
CONV3D_CONCAT_CASES = {
    "ztaps_concat_8_8_D2": (8, 8, 16, 2, 2, 9, 20, "0", 8),
    "ztaps_concat_32_32_D5": (32, 32, 32, 1, 5, 13, 20, "1", 32),
    "ztaps_concat_24_40_D1": (24, 40, 64, 2, 1, 17, 20, "1", 32),
}


def _conv3d_64(x, w, bias, post_relu):
    """NDHWC float64: explicit zero padding of all three axes, then the bare 27-tap sum."""
    N, D, H, W, C = x.shape
    xp = torch.zeros(N, D + 2, H + 2, W + 2, C, dtype=torch.float64)
    xp[:, 1:-1, 1:-1, 1:-1] = x.double()
    y = F.conv3d(xp.permute(0, 4, 1, 2, 3), w.double()).permute(0, 2, 3, 4, 1) + bias.double()
    mag = F.conv3d(xp.abs().permute(0, 4, 1, 2, 3), w.abs().double()).max().item()
    assert mag + 4 < 2 ** 22
    return rne(y.clamp_min(0.0) if post_relu else y).contiguous(), (rne(y).double() != y).double().mean().item()


def conv3d_data(name: str, monkeypatch) -> SimpleNamespace:
    """Sets the z-tap path's switches before the weights are packed (they are read at packing time)."""
    from bioengine_worker_amd.ops.conv3d import PackedConv3d

    if name in CONV3D_CASES:
        cin, cout, N, D, H, W, ck16, ck, post_relu = CONV3D_CASES[name]
        ca = None
    else:
        ca, cb, cout, N, D, H, W, ck16, ck = CONV3D_CONCAT_CASES[name]
        cin, post_relu = ca + cb, True
    monkeypatch.setenv("BE_CONV3D", "ztaps")
    monkeypatch.setenv("BE_CONV3D_CK16", ck16)
    monkeypatch.setenv("BE_CONV3D_NARROW", "1")
    g = torch.Generator().manual_seed(3000 + cin * 7 + D)
    w = _ri(g, -2, 2, cout, cin, 3, 3, 3)
    bias = _ri(g, -4, 4, cout)
    pc = PackedConv3d(w, bias)
    assert pc.cin_pad == cin and pc.ztap.ck == ck and pc.ztap.cin_pad == 3 * cin, (pc.cin_pad, pc.ztap.ck)
    x = (_ri(g, -6, 6, N, D, H, W, cin) / 2).bfloat16()
    want, frac = _conv3d_64(x, w, bias, post_relu)
    return SimpleNamespace(x=x, pc=pc, want=want, frac=frac, post_relu=post_relu, ca=ca)


# ------------------------------------------------------------------------------- the fused families
# The ping-pong kernels are proven bit for bit against the per-layer kernel elsewhere; here the same
# integer data ties them to the float64 model directly.  These convs DO build their fragment weights.

#: 3x3 128 -> 128 on conv_pp128 (forced grid): exact tiles of 8 x 28, and an interior tile plus partial ones
PP128_CASES = [
    Case("pp128_16x56_residual_strided_shift", cin=128, cout=128, H=16, W=56, res=True, shift="strided", rounds=True,
         seed=700),
    Case("pp128_24x60_shared_shift", cin=128, cout=128, H=24, W=60, shift="shared", rounds=True, seed=701),
    Case("pp128_24x60_out_aliases_residual", cin=128, cout=128, H=24, W=60, res=True, out="alias", rounds=True, seed=702),
]
#: the pooled build's 3x3 64 -> 128 conv and the 1x1 projection of the same pooled pixels
POOL_CONV = Case("pp128_pool_10x30", cin=64, cout=128, H=10, W=30, inmode="pool2", shift="strided", seed=710)
POOL_PROJ = Case("pp128_pool_proj_10x30", ks=1, cin=64, cout=128, H=10, W=30, inmode="pool2", shift="shared", relu=False,
                 seed=711)


def pool_pair():
    """(3x3 conv, 1x1 projection) over one source image."""
    dc, dp = make(POOL_CONV), make(POOL_PROJ)
    dp.x = dc.x
    dc.want, dp.want = ref64(dc), ref64(dp)
    return dc, dp


#: conv_pair's configurations (tests/test_conv_pair.py) at its tests' smallest shape:
#: Cin, CM, inmode, x2, proj, res, tA per image, tB per image
PAIR_CASES = [
    (8, 32, "none", False, True, "none", False, False),
    (32, 32, "none", False, False, "full", False, False),
    (32, 32, "none", False, False, "full", True, True),
    (64, 32, "up2", True, False, "up2", False, True),
    (32, 64, "pool2", False, False, "full", False, False),
    (64, 64, "none", False, False, "full", True, True),
    (128, 64, "up2", True, False, "up2", False, True),
]
PAIR_HW = (30, 44)


def pair_data(i: int) -> SimpleNamespace:
    """One fused half-block on integer data.  conv A is sparse (about 40 weights per output) so that the
    intermediate ``h = relu((convA(a) + x2) * sB + tB)`` stays a bf16 number (a multiple of 0.5 below
    128, asserted); conv B is dense, so its outputs round."""
    from bioengine_worker_amd.ops import conv_pair as cp
    from bioengine_worker_amd.ops.conv import PackedConv

    cin, cm, inmode, has_x2, proj, res_mode, ta2d, tb2d = PAIR_CASES[i]
    g = torch.Generator().manual_seed(4000 + i)
    N, (H, W) = 3, PAIR_HW
    Hs, Ws = {"none": (H, W), "pool2": (2 * H, 2 * W), "up2": (H // 2, W // 2)}[inmode]
    wa = _ri(g, -2, 2, cm, cin, 3, 3) * (torch.rand(cm, cin, 3, 3, generator=g) < 40.0 / (9 * cin))
    wb = _ri(g, -2, 2, cm, cm, 3, 3)
    x = _ri(g, -3, 3, N, Hs, Ws, cin).bfloat16()
    sa, sb = 2.0 ** _ri(g, -1, 1, cin), 2.0 ** _ri(g, -1, 0, cm)
    ta = _ri(g, -2, 2, N, cin) if ta2d else _ri(g, -2, 2, cin)
    tb = _ri(g, -2, 2, N, cm) if tb2d else _ri(g, -2, 2, cm)
    ta[..., 0], tb[..., 0] = 2.0, 1.0
    wa[:, 0] = 1.0
    bias = _ri(g, -4, 4, cm)
    x2 = _ri(g, -2, 2, N, H, W, cm).bfloat16() if has_x2 else None
    res = None
    if res_mode == "full":
        res = _ri(g, -8, 8, N, H, W, cm).bfloat16()
    elif res_mode == "up2":
        res = _ri(g, -8, 8, N, H // 2, W // 2, cm).bfloat16()
    kw = {}
    if proj:
        wp = _ri(g, -2, 2, cm, cin, 1, 1)
        kw = dict(pp=PackedConv.from_weight(wp, None), sp=2.0 ** _ri(g, -1, 1, cin), tp=_ri(g, -2, 2, cin))
    spec = cp.PairSpec(pa=PackedConv.from_weight(wa, None), pb=PackedConv.from_weight(wb, None), sa=sa, ta=None,
                       sb=sb, tb=None, bias=bias, inmode=inmode, **kw)
    # the float64 model
    iy, ix = torch.arange(H), torch.arange(W)
    xs = x.double()
    if inmode == "up2":
        xs = xs[:, iy // 2][:, :, ix // 2]
    elif inmode == "pool2":
        q = [xs[:, 2 * iy + dy][:, :, 2 * ix + dx] for dy in (0, 1) for dx in (0, 1)]
        xs = torch.maximum(torch.maximum(q[0], q[1]), torch.maximum(q[2], q[3]))
    a = (xs * sa.double() + _rows(ta, N)).clamp_min(0.0)
    assert torch.equal(a, a.to(torch.bfloat16).double())
    hA = conv64(padded(a, 3), wa)
    if x2 is not None:
        hA = hA + x2.double()
    h = (hA * sb.double() + _rows(tb, N)).clamp_min(0.0)
    assert torch.equal(h, h.to(torch.bfloat16).double()), f"pair {i}: h up to {h.max().item()} is no bf16 number"
    assert h.unique().numel() > 50
    y = conv64(padded(h, 3), wb)
    mag = conv64(padded(h, 3), wb.abs()).max().item()
    if proj:
        p = xs * kw["sp"].double() + kw["tp"].double()
        y = y + conv64(p, wp)
        mag += conv64(p.abs(), wp.abs()).max().item()
    y = y + bias.double()
    if res is not None:
        y = y + (res.double()[:, iy // 2][:, :, ix // 2] if res_mode == "up2" else res.double())
    assert mag + 12 < 2 ** 22
    frac = (rne(y).double() != y).double().mean().item()
    assert 0.05 <= frac <= 0.95 and rne(y).unique().numel() >= 100, (i, frac)
    return SimpleNamespace(x=x, x2=x2, res=res, res_mode=res_mode, ta=ta, tb=tb, spec=spec, want=rne(y), frac=frac)
