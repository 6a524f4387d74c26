"""Integer data for the linear-tile implicit-GEMM 3x3 conv (``csrc/kernels/conv_igemm.hip``,
``ops/conv_igemm.py``) and its alternative ``gemm_pp.conv3`` (``csrc/kernels/gemm_pp.hip``), and an
independent float64 model of one launch.  Tests compare with ``torch.equal``.

The model of one launch (shares no code with ``ops/conv_igemm.py`` or ``ops/gemm_pp.py``)::

    y    = conv64(padded(x, 3), w) + bias + residual      (bias / residual optional)
    out  = rne(relu(y) if post_relu else y)
    v    = out * ascale + ashift[n]                        (either optional; 1 and 0 when absent)
    aout = rne(relu(v) if arelu else v)                    (exists iff ascale or ashift is given)

Why equality is legitimate.  ``x`` (the already activated input) holds multiples of 0.5 in [-3, 3], ``w``
integers in [-2, 2] kept with probability ``dens``, ``bias`` integers in [-4, 4], ``residual`` integers in
[-8, 8], ``ascale`` 0.5, 1 or 2 and ``ashift`` multiples of 0.5 in [-4, 4] (as ``[Cout]``, ``[N, Cout]`` or
a column slice at offset 32 of ``[N, Cout + 64]``, which is how the style shifts arrive).  Every operand is a
bf16 number, every product a multiple of ``q`` = 0.5, and ``sum |x||w| + |bias| + |res| < 2^22 q``: fp32 is
exact in any order of summation.  ``v`` is an fp32 number, so the kernel's ``fmaf`` does not round either,
and the only roundings left are the two casts.  :func:`check_exactness` asserts all of it on the model.

What rounds (measured on the model; ``out``: share of outputs the first cast rounds, ``2nd``: share of ALL
outputs that are positive and produced by a second cast that rounds; ``rounds``: the case carries
``rounds=True``)::

    case                                            channels    geometry      out      2nd
    geom_5x8x8_tile_spans_four_images                32 -> 128  5 x 8 x 8      0.1 %    0.9 %
    geom_5x7x9_nothing_a_multiple_of_8               64 -> 128  5 x 7 x 9      1.6 %    2.8 %
    geom_2x13x17_seam_in_mid_row                     32 -> 128  2 x 13 x 17     0.2 %    1.1 %
    geom_3x28x28_level3                              64 -> 128  3 x 28 x 28     2.0 %    2.4 %
    geom_1x1x1_rows_clamp_2d_shift_of_one_image      32 -> 128  1 x 1 x 1      0.0 %    0.0 %
    geom_1x3x5_rows_clamp                            64 -> 128  1 x 3 x 5      0.9 %    1.6 %
    geom_1x40x1_one_column_2d_shift_of_one_image     32 -> 128  1 x 40 x 1      0.0 %    0.1 %
    geom_1x1x40_one_row                              64 -> 128  1 x 1 x 40     0.1 %    0.6 %
    geom_7x3x5_one_ragged_tile_over_seven_images     32 -> 128  7 x 3 x 5      0.1 %    0.6 %
    chunks1_cin16                                    16 -> 128  2 x 13 x 17     0.0 %    0.3 %
    chunks2_cin32                                    32 -> 128  2 x 13 x 17     0.2 %    1.1 %
    chunks3_cin48                                    48 -> 128  2 x 13 x 17     0.9 %    1.8 %
    chunks4_cin64                                    64 -> 128  2 x 13 x 17     1.8 %    3.6 %
    chunks8_cin128                                  128 -> 128  2 x 13 x 17     6.9 %    5.2 %  rounds
    chunks16_cin256                                 256 -> 128  2 x 13 x 17    15.7 %    8.8 %  rounds
    blocks_cout64_5x8x8                              32 ->  64  5 x 8 x 8      0.1 %    0.9 %
    blocks_cout192_2x13x17                           32 -> 192  2 x 13 x 17     0.2 %    1.3 %
    blocks_cout192_3x28x28                           16 -> 192  3 x 28 x 28     0.0 %    0.4 %
    blocks_cout256_4x16x16                           32 -> 256  4 x 16 x 16     0.2 %    1.0 %
    blocks_cout256_3x28x28_cin256_level3            256 -> 256  3 x 28 x 28    16.0 %    8.8 %  rounds
    epi128_bias_none                                128 -> 128  2 x 13 x 17     6.7 %    4.8 %  rounds
    epi128_residual_none                            128 -> 128  2 x 13 x 17     6.7 %    5.7 %  rounds
    epi128_aout_only_with_residual                  128 -> 128  2 x 13 x 17     6.7 %    4.6 %  rounds
    epi128_aout_only_no_residual                    128 -> 128  2 x 13 x 17     6.7 %    6.1 %  rounds
    epi128_post_relu                                128 -> 128  2 x 13 x 17     3.4 %    4.5 %
    epi128_arelu_false                              128 -> 128  2 x 13 x 17     6.9 %    6.4 %  rounds
    epi128_ascale_alone                             128 -> 128  2 x 13 x 17     6.9 %    0.0 %  rounds
    epi128_ashift_alone                             128 -> 128  2 x 13 x 17     6.9 %    3.1 %  rounds
    epi128_shift_shared                             128 -> 128  2 x 13 x 17     6.9 %    4.3 %  rounds
    epi128_shift_rows_contiguous                    128 -> 128  2 x 13 x 17     6.7 %    4.9 %  rounds
    epi128_shift_strided                            128 -> 128  2 x 13 x 17     7.0 %    5.3 %  rounds
    epi128_out_and_aout_given                       128 -> 128  2 x 13 x 17     6.6 %    5.0 %  rounds
    epi128_no_activation                            128 -> 128  2 x 13 x 17     6.8 %    0.0 %  rounds
    epi256_bias_none                                256 -> 256  5 x 8 x 8     14.1 %    7.4 %  rounds
    epi256_residual_none                            256 -> 256  5 x 8 x 8     14.0 %    7.6 %  rounds
    epi256_aout_only_with_residual                  256 -> 256  5 x 8 x 8     14.0 %    7.5 %  rounds
    epi256_aout_only_no_residual                    256 -> 256  5 x 8 x 8     14.2 %    8.1 %  rounds
    epi256_post_relu                                256 -> 256  5 x 8 x 8      7.1 %    7.3 %  rounds
    epi256_arelu_false                              256 -> 256  5 x 8 x 8     14.0 %    8.0 %  rounds
    epi256_ascale_alone                             256 -> 256  5 x 8 x 8     13.9 %    0.0 %  rounds
    epi256_ashift_alone                             256 -> 256  5 x 8 x 8     14.2 %    6.7 %  rounds
    epi256_shift_shared                             256 -> 256  5 x 8 x 8     14.1 %    8.3 %  rounds
    epi256_shift_rows_contiguous                    256 -> 256  5 x 8 x 8     14.1 %    8.2 %  rounds
    epi256_shift_strided                            256 -> 256  5 x 8 x 8     14.1 %    8.8 %  rounds
    epi256_out_and_aout_given                       256 -> 256  5 x 8 x 8     14.0 %    7.4 %  rounds
    epi256_no_activation                            256 -> 256  5 x 8 x 8     14.0 %    0.0 %  rounds
    pp_cin96_three_k_halves_per_tap                  96 -> 128  2 x 13 x 17     4.1 %    4.1 %
    pp_cout68_ragged_n                               32 ->  68  5 x 7 x 9      0.1 %    0.9 %
    pp_cout132_ragged_n                              64 -> 132  2 x 13 x 17     1.9 %    2.9 %

The worst-case magnitude ``sum |x||w| + |bias| + |res|`` is at most 0.0023 of ``2^22 q``.  The chained route
models (below) reach 0.17 (down, the dense last conv) and 0.07 (up) of their launches' own ``2^22 q``, with
92 % and 91 % of the final outputs rounded.

Rounding cases must have 5 % .. 95 % of ``out`` rounded, at least 100 distinct values and, where a shift is
given, a ``2nd`` share of at least 3 %.  Without a shift the second cast cannot round at all: ``out`` is a
bf16 number and ``ascale`` a power of two, so ``v`` is a bf16 number; such cases must have a share of exactly
0.  ``epi128_post_relu`` does not carry the mark: the output ReLU clamps half of its outputs, and 3.4 % are left
that round.  The other cases pin indexing and must hold ``min(100, numel / 4)`` distinct values.  The table is
printed by ``python tests/conv_igemm_exact_cases.py``.

The chained model of the engine's level-3 routes (:func:`down_model`, :func:`up_model`) follows ``resdown`` /
``resup`` of ``models/cpnet.py`` launch by launch, one ``rne`` per stored tensor and two for an activated
copy, and checks every launch with that launch's own quantum (:func:`quantum`).
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from types import SimpleNamespace

import torch

from conv_exact_cases import _ri, conv64, padded, rne, tap_code, trunc

Q = 0.5
MAG_LIMIT = 1.0  # of 2^22 q: the worst-case partial sum of a launch
BNS = (64, 65, 128, 1065, 1128)  # conv3_igemm's builds: + 1000 = three stage buffers
PP_TILES = {0: (256, 256), 1: (512, 128), 2: (256, 128)}  # gemm_pp.conv3's cfg -> (pixels, channels) per tile


def bm_of(bn: int) -> int:
    """Consecutive pixels per tile."""
    return 512 if bn % 1000 == 65 else 256


def bnc_of(bn: int) -> int:
    """Output channels per block."""
    return 128 if bn % 1000 == 128 else 64


@dataclass(frozen=True)
class Case:
    name: str
    N: int
    H: int
    W: int
    cin: int = 32
    cout: int = 128
    bias: bool = True
    res: bool = True
    want_out: bool = True
    post_relu: bool = False
    arelu: bool = True
    ascale: bool = True
    ashift: str | None = "strided"  # None | shared [Cout] | rows [N, Cout] | strided (columns 32.. of [N, Cout + 64])
    given: bool = False             # out= / aout= handed in, pre-filled with 77
    dens: float = 1.0
    rounds: bool = False
    seed: int = 0

    @property
    def bns(self) -> tuple:
        """The conv3_igemm builds this Cout admits (every geometry of the list fits every build's halo)."""
        return tuple(b for b in BNS if self.cout % bnc_of(b) == 0)

    @property
    def act(self) -> bool:
        return self.ascale or self.ashift is not None


def make(case: Case) -> SimpleNamespace:
    """The seeded draws of one case as CPU tensors, with the exact sum ``y`` and the answer ``want``."""
    g = torch.Generator().manual_seed(7000 + case.seed)
    N, H, W, cin, cout = case.N, case.H, case.W, case.cin, case.cout
    w = _ri(g, -2, 2, cout, cin, 3, 3)
    w = w * (torch.rand(w.shape, generator=g) < case.dens)
    d = SimpleNamespace(case=case, w=w)
    d.x = (_ri(g, -6, 6, N, H, W, cin) / 2).bfloat16()
    d.bias = _ri(g, -4, 4, cout) if case.bias else None
    d.res = _ri(g, -8, 8, N, H, W, cout).bfloat16() if case.res else None
    d.ascale = 2.0 ** _ri(g, -1, 1, cout) if case.ascale else None
    half = lambda *s: _ri(g, -8, 8, *s) / 2
    d.ashift = {None: lambda: None, "shared": lambda: half(cout), "rows": lambda: half(N, cout),
                "strided": lambda: half(N, cout + 64)[:, 32:32 + cout]}[case.ashift]()
    d.y = presum(d)
    d.want = finish(d, d.y)
    return d


def _rows(t: torch.Tensor) -> torch.Tensor:
    """[C], [N, C] or [N, H, W, C] shift -> float64 broadcastable over NHWC."""
    t = t.double()
    return t[:, None, None, :] if t.dim() == 2 else t


def presum(d) -> torch.Tensor:
    """The exact float64 value in front of the first cast, NHWC."""
    y = conv64(padded(d.x.double(), 3), d.w)
    if d.bias is not None:
        y = y + d.bias.double()
    if d.res is not None:
        y = y + d.res.double()
    return y


def finish(d, y: torch.Tensor, cast1=rne, cast2=rne, shift=None, from_y: bool = False):
    """(out, aout) of the exact sum ``y``: the two casts.  The keyword arguments are the mutants' hooks."""
    c = d.case
    y = y.clamp_min(0.0) if c.post_relu else y
    out = cast1(y)
    if d.ascale is None and d.ashift is None:
        return out, None
    v = y if from_y else out.double()
    if d.ascale is not None:
        v = v * d.ascale.double()
    shift = d.ashift if shift is None else shift
    if shift is not None:
        v = v + _rows(shift)
    return out, cast2(v.clamp_min(0.0) if c.arelu else v)


def returned(d, pair) -> tuple:
    """What the launch hands back: ``out`` is None with ``want_out=False``, ``aout`` None without an activation."""
    out, aout = pair
    return (out if d.case.want_out else None), aout


def same(d, a, b) -> bool:
    a, b = returned(d, a), returned(d, b)
    return all((s is None and t is None) or torch.equal(s, t) for s, t in zip(a, b))


# ------------------------------------------------------------------------------------ preconditions


def quantum(*ts) -> float:
    """The largest power of two (at most 1) that divides every value of the given tensors."""
    k = 0
    ts = [t.double() for t in ts if t is not None]
    while any(not torch.equal(t * 2.0 ** k, (t * 2.0 ** k).round()) for t in ts):
        k += 1
        assert k < 64
    return 2.0 ** -k


def launch64(a, w, bias=None, res=None, ascale=None, ashift=None, *, post_relu=False, arelu=True, q=None, name=""):
    """The float64 model of one launch on the activated input ``a`` [N, H, W, Cin], with the conditions
    under which the kernel must reproduce it bit for bit asserted: bf16 operands, integer weights, products
    on the grid ``q`` (None: :func:`quantum` of the operands), worst-case magnitude below ``2^22 q``, and
    ``v`` an fp32 number.  -> y, out, aout, v, q, mag (as a share of ``2^22 q``)."""
    a = a.double()
    bf = lambda t: torch.equal(t.double(), t.to(torch.bfloat16).double())
    for nm, t in (("input", a), ("weight", w), ("residual", res)):  # what the kernel reads as bf16 ...
        assert t is None or bf(t), f"{name}: the {nm} holds a value that is no bf16 number"
    for nm, t in (("bias", bias), ("ascale", ascale), ("ashift", ashift)):  # ... and as fp32
        assert t is None or torch.equal(t.double(), t.float().double()), f"{name}: the {nm} is no fp32 number"
    assert torch.equal(w, w.round()), f"{name}: a weight is no integer"
    q = quantum(a, bias, res) if q is None else q
    for t in (a, bias, res):
        assert t is None or torch.equal(t.double() / q, (t.double() / q).round()), f"{name}: a term is off the grid {q}"
    ks = w.shape[-1]
    ap = padded(a, ks)
    y, mag = conv64(ap, w), conv64(ap.abs(), w.abs())
    if bias is not None:
        y, mag = y + bias.double(), mag + bias.double().abs()
    if res is not None:
        y, mag = y + res.double(), mag + res.double().abs()
    share = mag.max().item() / (2.0 ** 22 * q)
    assert share < MAG_LIMIT, f"{name}: a partial sum may leave the exact range of fp32 ({share:.3f} of 2^22 q)"
    yr = y.clamp_min(0.0) if post_relu else y
    out = rne(yr)
    v = aout = None
    if ascale is not None or ashift is not None:
        v = out.double() * (1.0 if ascale is None else ascale.double())
        v = v + (0.0 if ashift is None else _rows(ashift))
        assert torch.equal(v.float().double(), v), f"{name}: the activated value is no fp32 number (fmaf would round)"
        aout = rne(v.clamp_min(0.0) if arelu else v)
    return SimpleNamespace(y=y, yr=yr, out=out, v=v, aout=aout, q=q, mag=share)


def check_exactness(d) -> dict:
    """The conditions under which equality may be demanded of this case, checked on the model alone."""
    c = d.case
    m = launch64(d.x, d.w, d.bias, d.res, d.ascale, d.ashift, post_relu=c.post_relu, arelu=c.arelu, q=Q, name=c.name)
    assert torch.equal(m.y, d.y) and same(d, (m.out, m.aout), d.want), f"{c.name}: two ways to the same model differ"
    for t in (d.x, d.w, d.bias, d.res, d.ascale, d.ashift):
        assert t is None or torch.equal(t.double(), rne(t).double()), f"{c.name}: an operand is no bf16 number"
    frac = (m.out.double() != m.yr).double().mean().item()
    frac2 = 0.0 if m.v is None else ((m.v > 0) & (rne(m.v).double() != m.v)).double().mean().item()
    distinct = m.out.unique().numel()
    if c.rounds:
        assert c.cin >= 128 and c.dens == 1.0
        assert 0.05 <= frac <= 0.95, f"{c.name}: {frac:.3f} of the outputs round (want 5 % .. 95 %)"
        assert distinct >= 100, f"{c.name}: {distinct} distinct outputs"
        if d.ashift is not None:
            assert frac2 >= 0.03, f"{c.name}: {frac2:.3f} of the outputs are positive with a rounding second cast"
        else:  # bf16 times a power of two is a bf16 number
            assert frac2 == 0.0
    else:
        assert distinct >= min(100, m.out.numel() // 4), f"{c.name}: {distinct} distinct outputs of {m.out.numel()}"
    return dict(frac=frac, frac2=frac2, distinct=distinct, mag=m.mag)


# --------------------------------------------------------------------------------- mismatch report


def assert_exact_linear(got: torch.Tensor, want: torch.Tensor, name: str, bm: int = 256, bnc: int = 64):
    """``torch.equal`` with a report for linear tiles: count, first (n, y, x, co), expected and got, linear
    pixel ``m``, tile ``m // bm``, in-tile offset and wave ``offset // 64``, channel block ``co // bnc``."""
    assert got.shape == want.shape, f"{name}: shape {tuple(got.shape)} != {tuple(want.shape)}"
    assert got.dtype == want.dtype, f"{name}: dtype {got.dtype} != {want.dtype}"
    g, w = got.double().cpu(), want.double().cpu()
    bad = g != w
    if not bad.any():
        return
    N, H, W, C = w.shape
    idx = bad.nonzero()
    first = tuple(idx[0].tolist())
    n, y, x, co = first
    m = (n * H + y) * W + x
    ms = (idx[:, 0] * H + idx[:, 1]) * W + idx[:, 2]
    tiles = sorted(set((ms // bm).tolist()))
    blocks = sorted(set((idx[:, 3] // bnc).tolist()))
    raise AssertionError(
        f"{name}: {int(bad.sum())} of {bad.numel()} outputs differ; first at (n, y, x, co) = {first}: expected "
        f"{w[first].item()}, got {g[first].item()}; linear pixel m = {m}, tile m // {bm} = {m // bm}, in-tile offset "
        f"{m % bm} (wave {m % bm // 64}), channel block co // {bnc} = {co // bnc} (+{co % bnc}); tiles hit: "
        f"{tiles[:12]} of {(N * H * W + bm - 1) // bm}, channel blocks hit: {blocks[:8]}")


def assert_pair_exact(d, got, name: str, bm: int = 256, bnc: int = 64):
    """Both returned tensors of a launch against the case's answer."""
    for what, g, w in zip(("out", "aout"), got, returned(d, d.want)):
        assert (g is None) == (w is None), f"{name}: {what} is {'missing' if g is None else 'unexpected'}"
        if w is not None:
            assert_exact_linear(g, w, f"{name} {what}", bm=bm, bnc=bnc)


# ------------------------------------------------------------------------------------------- mutants
# Faults of the kind this kernel can have, injected into the float64 model.  Each returns the mutated
# (out, aout), or None where the case does not offer the fault.  ``bm``: pixels per linear tile.


def mut_truncate_first_cast(d, bm):
    return finish(d, d.y, cast1=trunc)


def mut_truncate_second_cast(d, bm):
    return finish(d, d.y, cast2=trunc) if d.case.act else None


def mut_aout_from_unrounded_y(d, bm):
    """The activated copy computed from the fp32 sum and not from the rounded ``out``: one cast, not two."""
    return finish(d, d.y, from_y=True) if d.case.act else None


def mut_pad_row_is_next_image(d, bm):
    """The padded row below the last row of image n holds row 0 of image n + 1: a halo that runs on."""
    c = d.case
    if c.N < 2:
        return None
    n = c.N - 2
    ap = padded(d.x.double()[n:n + 1], 3)[:, c.H - 1:]  # the three padded rows under output row H - 1
    bad = ap.clone()
    bad[0, 2, 1:c.W + 1] = d.x.double()[n + 1, 0]
    y = d.y.clone()
    y[n, c.H - 1] += (conv64(bad, d.w) - conv64(ap, d.w))[0, 0]
    return finish(d, y)


def mut_shift_of_tiles_first_image(d, bm):
    """Every pixel of a tile takes the shift row of the image the tile starts in."""
    c = d.case
    if d.ashift is None or d.ashift.dim() != 2 or c.N < 2:
        return None
    m = torch.arange(c.N * c.H * c.W)
    first = (m // bm * bm) // (c.H * c.W)
    if torch.equal(first, m // (c.H * c.W)):
        return None  # no tile crosses an image boundary
    return finish(d, d.y, shift=d.ashift.double()[first].reshape(c.N, c.H, c.W, c.cout))


def _halo_index(c, m, bm):
    """Index of pixel ``m`` in the halo of its tile, as the kernel counts it: padded rows from the tile's
    first (one above the tile's first output row), W + 2 pixels each."""
    HW, H2, W2 = c.H * c.W, c.H + 2, c.W + 2
    m0 = m // bm * bm
    n0, y0 = m0 // HW, m0 % HW // c.W
    n, y, x = m // HW, m % HW // c.W, m % c.W
    return (n * H2 + y + 1 - (n0 * H2 + y0)) * W2 + x + 1


def mut_halo_halves_swapped(d, bm):
    """Channels 0-7 and 8-15 of the last K chunk swapped at one halo pixel of an odd group of 8 (where the
    LDS image swaps the two halves), for the tile that stages it."""
    c = d.case
    NP, HW = c.N * c.H * c.W, c.H * c.W
    hit = [m for m in range(min(bm, NP)) if (_halo_index(c, m, bm) >> 3) & 1]
    if not hit:
        return None
    m = hit[len(hit) // 2]
    n, yy, xx = m // HW, m % HW // c.W, m % c.W
    k = slice(c.cin - 16, c.cin)
    a = d.x.double()[n:n + 1, :, :, k]
    bad = a.clone()
    bad[0, yy, xx, :8], bad[0, yy, xx, 8:] = a[0, yy, xx, 8:], a[0, yy, xx, :8]
    delta = (conv64(padded(bad, 3), d.w[:, k]) - conv64(padded(a, 3), d.w[:, k])).reshape(HW, c.cout)
    y = d.y.clone()
    rows = y.view(NP, c.cout)
    hi = min((n + 1) * HW, bm)  # the pixels of image n inside tile 0
    rows[n * HW:hi] += delta[:hi - n * HW]
    return finish(d, y)


def mut_stale_k_chunk(d, bm):
    """The last K chunk of the last tile replaced by the chunk two before it, weights and halo alike: a
    stage buffer read before its DMA landed."""
    c = d.case
    nch = c.cin // 16
    if nch < 3:
        return None
    NP = c.N * c.H * c.W
    t = (NP - 1) // bm
    cur, old = slice(16 * (nch - 1), 16 * nch), slice(16 * (nch - 3), 16 * (nch - 2))
    ap = padded(d.x.double(), 3)
    delta = (conv64(ap[..., old].contiguous(), d.w[:, old]) - conv64(ap[..., cur].contiguous(), d.w[:, cur]))
    y = d.y.clone()
    y.view(NP, c.cout)[t * bm:(t + 1) * bm] += delta.reshape(NP, c.cout)[t * bm:(t + 1) * bm]
    return finish(d, y)


def mut_residual_of_next_pixel(d, bm):
    """The last lane of the first wave adds the residual of pixel m + 1."""
    c = d.case
    NP = c.N * c.H * c.W
    if d.res is None or NP < 2:
        return None
    m = min(63, NP - 2)
    r = d.res.double().reshape(NP, c.cout)
    y = d.y.clone()
    y.view(NP, c.cout)[m] += r[m + 1] - r[m]
    return finish(d, y)


def mut_drop_product(d, bm):
    """One (pixel, tap, channel) product missing from one output."""
    c = d.case
    ap = padded(d.x.double(), 3)
    n, yy, xx = c.N - 1, c.H // 2, c.W // 2
    prod = ap[n, yy:yy + 3, xx:xx + 3, :].permute(2, 0, 1)[None] * d.w.double()  # [co, ci, ty, tx]
    hit = prod.nonzero()
    if not len(hit):
        return None
    co, ci, ty, tx = hit[len(hit) // 2].tolist()
    y = d.y.clone()
    y[n, yy, xx, co] -= prod[co, ci, ty, tx]
    return finish(d, y)


MUTANTS = {
    "truncate_first_cast": mut_truncate_first_cast,
    "truncate_second_cast": mut_truncate_second_cast,
    "aout_from_unrounded_y": mut_aout_from_unrounded_y,
    "pad_row_is_next_image": mut_pad_row_is_next_image,
    "shift_of_tiles_first_image": mut_shift_of_tiles_first_image,
    "halo_halves_swapped": mut_halo_halves_swapped,
    "stale_k_chunk": mut_stale_k_chunk,
    "residual_of_next_pixel": mut_residual_of_next_pixel,
    "drop_product": mut_drop_product,
}


# --------------------------------------------------------------------------------------------- cases


def _geometry_cases():
    geo = [
        ("5x8x8_tile_spans_four_images", 5, 8, 8, "strided"),
        ("5x7x9_nothing_a_multiple_of_8", 5, 7, 9, "strided"),
        ("2x13x17_seam_in_mid_row", 2, 13, 17, "strided"),
        ("3x28x28_level3", 3, 28, 28, "strided"),
        ("1x1x1_rows_clamp_2d_shift_of_one_image", 1, 1, 1, "rows"),
        ("1x3x5_rows_clamp", 1, 3, 5, "strided"),
        ("1x40x1_one_column_2d_shift_of_one_image", 1, 40, 1, "rows"),
        ("1x1x40_one_row", 1, 1, 40, "strided"),
        ("7x3x5_one_ragged_tile_over_seven_images", 7, 3, 5, "strided"),
    ]
    return [Case(f"geom_{nm}", N, H, W, cin=(32, 64)[i % 2], cout=128, ashift=sh, seed=i)
            for i, (nm, N, H, W, sh) in enumerate(geo)]


def _chunk_cases():
    """Cin / 16 K chunks: 1 (the three-stage builds' ``nchunk > 1`` guard), 2, 3, 4, 8 and 16 (every stage
    buffer reused several times)."""
    return [Case(f"chunks{cin // 16}_cin{cin}", 2, 13, 17, cin=cin, cout=128, rounds=cin >= 128, seed=20 + i)
            for i, cin in enumerate((16, 32, 48, 64, 128, 256))]


def _block_cases():
    """Output blocks and block order (``xcd_remap``): ``tiles * Cout / bnc`` below 8, above 8 and no multiple
    of 8, and a multiple of 8, on every build (``test_block_counts`` asserts it)."""
    return [
        Case("blocks_cout64_5x8x8", 5, 8, 8, cin=32, cout=64, seed=40),
        Case("blocks_cout192_2x13x17", 2, 13, 17, cin=32, cout=192, seed=41),
        Case("blocks_cout192_3x28x28", 3, 28, 28, cin=16, cout=192, seed=42),
        Case("blocks_cout256_4x16x16", 4, 16, 16, cin=32, cout=256, seed=43),
        Case("blocks_cout256_3x28x28_cin256_level3", 3, 28, 28, cin=256, cout=256, rounds=True, seed=44),
    ]


def _epilogue_cases():
    out = []
    variants = [
        ("bias_none", dict(bias=False)),
        ("residual_none", dict(res=False)),
        ("aout_only_with_residual", dict(want_out=False)),
        ("aout_only_no_residual", dict(want_out=False, res=False)),
        ("post_relu", dict(post_relu=True)),
        ("arelu_false", dict(arelu=False)),
        ("ascale_alone", dict(ashift=None)),
        ("ashift_alone", dict(ascale=False)),
        ("shift_shared", dict(ashift="shared")),
        ("shift_rows_contiguous", dict(ashift="rows")),
        ("shift_strided", dict(ashift="strided")),
        ("out_and_aout_given", dict(given=True)),
        ("no_activation", dict(ascale=False, ashift=None)),
    ]
    for ch, (N, H, W) in ((128, (2, 13, 17)), (256, (5, 8, 8))):
        for i, (nm, kw) in enumerate(variants):
            # the output ReLU clamps half of the outputs: at 128 channels 3.4 % are left that round, which is
            # below the 5 % a rounding case must show, so that one case does not carry the mark
            rounds = not (ch == 128 and kw.get("post_relu"))
            out.append(Case(f"epi{ch}_{nm}", N, H, W, cin=ch, cout=ch, rounds=rounds, seed=100 + ch + i, **kw))
    return out


@functools.lru_cache(maxsize=None)
def cases() -> tuple:
    out = _geometry_cases() + _chunk_cases() + _block_cases() + _epilogue_cases()
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


#: gemm_pp.conv3 alone: three K-halves per tap, and ragged N (the ``brow`` clamp and the ``nok`` guard)
PP_EXTRA = (
    Case("pp_cin96_three_k_halves_per_tap", 2, 13, 17, cin=96, cout=128, seed=60),
    Case("pp_cout68_ragged_n", 5, 7, 9, cin=32, cout=68, seed=61),
    Case("pp_cout132_ragged_n", 2, 13, 17, cin=64, cout=132, seed=62),
)


def pp_cases() -> tuple:
    return tuple(c for c in cases() if c.cin % 32 == 0) + PP_EXTRA


def by_name(name: str) -> Case:
    return next(c for c in cases() + PP_EXTRA if c.name == name)


@functools.lru_cache(maxsize=None)
def data(name: str) -> SimpleNamespace:
    """The case's draws and its answer, made once and shared; tests must not write to them."""
    return make(by_name(name))


def widest_case(bn: int, W: int) -> Case:
    """2 x 4 x W at Cin 16 for the widest-image tests (W comes from ``supported``)."""
    return Case(f"widest_bn{bn}_W{W}", 2, 4, W, cin=16, cout=bnc_of(bn), seed=80 + bn % 7 + W)


# ------------------------------------------------------------------------------------------ running


def _kwargs(d, device, mv):
    c = d.case
    shift = d.ashift
    if shift is not None and not shift.is_contiguous():  # stays a column slice of its wide parent on the device
        shift = mv(shift._base)[:, 32:32 + c.cout]
        assert not shift.is_contiguous() or c.N == 1
    else:
        shift = mv(shift)
    kw = dict(residual=mv(d.res), want_out=c.want_out, ascale=mv(d.ascale), ashift=shift, arelu=c.arelu,
              post_relu=c.post_relu)
    given = {}
    if c.given:
        full = lambda: torch.full((c.N, c.H, c.W, c.cout), 77.0, dtype=torch.bfloat16, device=device or "cpu")
        given = dict(out=full() if c.want_out else None, aout=full() if c.act else None)
    return kw, given


def _back(got, given, on_device):
    out, aout = got
    if on_device:  # the CPU paths are the fp32 formulas and allocate their results
        for k, t in (("out", out), ("aout", aout)):
            if given.get(k) is not None:
                assert t is given[k], f"the given {k}= must be the returned tensor"
    return (None if out is None else out.cpu()), (None if aout is None else aout.cpu())


def run_igemm(d, device=None, bn: int = 64):
    """``conv3_igemm`` of the case on ``device`` (None: the CPU path) -> (out, aout) on the CPU."""
    from bioengine_worker_amd.ops import conv_igemm as ig

    mv = (lambda t: t) if device is None else (lambda t: None if t is None else t.to(device))
    pk = ig.IgemmConv.from_weight(d.w, d.bias, bn=bn)
    assert pk.bnc == bnc_of(bn)
    if device is not None:
        pk = pk.to(device)
    kw, given = _kwargs(d, device, mv)
    got = ig.conv3_igemm(mv(d.x), pk, **kw, **given)
    return _back(got, given, device is not None)


def run_pp(d, device=None, cfg: int = 0):
    """``gemm_pp.conv3`` of the same data."""
    from bioengine_worker_amd.ops import gemm_pp as pp

    mv = (lambda t: t) if device is None else (lambda t: None if t is None else t.to(device))
    kw, given = _kwargs(d, device, mv)
    got = pp.conv3(mv(d.x), mv(pp.pack_conv3(d.w)), mv(d.bias), cfg=cfg, **kw, **given)
    return _back(got, given, device is not None)


# ----------------------------------------------------------------------------------------- tap map

TAP_SHAPE = (13, 17, 32, 128)  # H, W, Cin, Cout
TAP_BNS = (64, 128, 1065)


@functools.lru_cache(maxsize=None)
def tap_map():
    """One image per (position, input channel), all in one batch so that tiles cross images; each holds a
    single 1 and the weights are ``tap_code``.  -> (x bf16, w, expected bf16, items): the flipped 3x3 stamp
    of codes around the 1 -- out[y - ty + 1, x - tx + 1, co] = w[co, ci, ty, tx] -- built by index, and zero
    elsewhere (in particular in the neighbouring images).  Positions: the four corners (the last pixel of
    an image and the first of the next among them), one pixel in each parity of ``(halo index >> 3) & 1``,
    and linear pixels 255 and 0 (mod 256) at either side of a tile seam (255, 512, 768, 1023, ...: an image
    holds one 1, so the two sides of one seam fall to different channels), placed in the images that hold
    them.  ``items``: (n, y, x, ci) of every 1."""
    H, W, cin, cout = TAP_SHAPE
    HW = H * W
    chans = [0, 7, 8, 15, 16, cin - 1]
    fixed = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (6, 3), (6, 11)]
    pend_fixed = [(p, ci) for p in fixed for ci in chans]
    # either side of a seam in turn, so that both sides also fall on the seams of the 512-pixel tiles
    pend_seam = [(r, ci) for i, ci in enumerate(chans) for r in ((255, 0), (0, 255))[i % 2]]
    items, n = [], 0
    while pend_fixed or pend_seam:
        lo = n * HW
        if pend_seam and lo + (pend_seam[0][0] - lo) % 256 < lo + HW:
            r, ci = pend_seam.pop(0)
            rem = (r - lo) % 256
            items.append((n, rem // W, rem % W, ci))
        elif pend_fixed:
            (y, x), ci = pend_fixed.pop(0)
            items.append((n, y, x, ci))
        n += 1  # an image that can hold neither stays empty
    N = n
    w = tap_code(cout, cin)
    x = torch.zeros(N, H, W, cin)
    want = torch.zeros(N, H, W, cout)
    for n, y, xx, ci in items:
        x[n, y, xx, ci] = 1.0
        for ty in range(3):
            for tx in range(3):
                oy, ox = y - ty + 1, xx - tx + 1
                if 0 <= oy < H and 0 <= ox < W:
                    want[n, oy, ox] = w[:, ci, ty, tx]
    return x.bfloat16(), w, want.bfloat16(), tuple(items)


def tap_halo_parities(bm: int) -> set:
    H, W, _, _ = TAP_SHAPE
    c = SimpleNamespace(H=H, W=W)
    return {(_halo_index(c, (n * H + y) * W + x, bm) >> 3) & 1 for n, y, x, _ in tap_map()[3]}


# ---------------------------------------------------------------------------- the level-3 routes
# A default CPnet whose deepest blocks carry integer parameters, and the float64 model of the engine's
# level-3 routes, chained launch by launch after ``resdown.forward`` / ``resup.forward``.

ROUTE_N, ROUTE_HW, ROUTE_C = 5, 8, 256  # src is [5, 16, 16, 128]; level 3 works on 5 x 8 x 8 x 256
#: Centres of the BatchNorm running means, per conv whose input the BatchNorm activates.  A sparse conv of
#: 40 weights multiplies the spread of its input by about 9 and a scale of 0.5 halves the quantum, so with
#: centred statistics the worst-case sum outgrows 2^22 quanta after three launches.  Means of about 1.3
#: standard deviations of the tensor they normalise (even integers, measured on the model) leave a tenth
#: of the activations positive and keep every launch below a fifth of that range.
ROUTE_MEANS = {"down": (0, 36, 104, 300), "up": (3000, 22, 80, 200)}


def _int_bn(bn, g, mean=0.0):
    """eps 0, weight 1, var in {0.25, 1, 4}: folded scale 2, 1 or 0.5; even means and integer bias: integer shift.
    ``mean``: the centre of the running means (:data:`ROUTE_MEANS`)."""
    C = bn.num_features
    bn.eps = 0.0
    bn.weight.data = torch.ones(C)
    bn.running_var.data = 4.0 ** _ri(g, -1, 1, C)
    bn.running_mean.data = mean + 2.0 * _ri(g, -1, 1, C)
    bn.bias.data = _ri(g, -2, 0, C)


def _int_conv(conv, g, per_output=None):
    """Integer weights in [-2, 2]; ``per_output``: about that many non-zero weights per output, None: dense."""
    w = _ri(g, -2, 2, *conv.weight.shape)
    if per_output is not None:
        fan = conv.weight[0].numel()
        w = w * (torch.rand(w.shape, generator=g) < per_output / (0.8 * fan))
    conv.weight.data = w
    conv.bias.data = _ri(g, -4, 4, conv.weight.shape[0])


@functools.lru_cache(maxsize=None)
def route_net():
    from bioengine_worker_amd.models.cpnet import CPnet

    net = CPnet().randomize_(5).eval()
    g = torch.Generator().manual_seed(9000)
    dn, up = net.downsample.down[3], net.upsample.up[3]
    assert dn.proj[1].weight.shape == (256, 128, 1, 1) and up.conv[0][2].weight.shape == (256, 256, 3, 3)
    for seq in (dn.proj, up.proj):
        _int_bn(seq[0], g)
        _int_conv(seq[1], g, 40)
    for k in range(4):
        _int_bn(dn.conv[k][0], g, ROUTE_MEANS["down"][k])
        _int_conv(dn.conv[k][2], g, None if k == 3 else 40)
        seq = up.conv[k] if k == 0 else up.conv[k].conv
        _int_bn(seq[0], g, ROUTE_MEANS["up"][k])
        _int_conv(seq[2], g, None if k == 3 else 40)
    return net


def bn64(bn):
    """Folded eval-mode BatchNorm in float64: (scale, shift)."""
    s = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
    return s, bn.bias.detach().double() - bn.running_mean.double() * s


def _bf16_number(t, name):
    assert torch.equal(t, t.to(torch.bfloat16).double()), f"{name} is no bf16 number"
    return t


def _conv_of(seq):
    return seq[-1].weight.detach(), seq[-1].bias.detach()


@functools.lru_cache(maxsize=None)
def route_inputs() -> SimpleNamespace:
    """Different tensors for everything the two route methods take."""
    g = torch.Generator().manual_seed(9001)
    N, S, C = ROUTE_N, ROUTE_HW, ROUTE_C
    half = lambda *s: (_ri(g, -6, 6, *s) / 2).bfloat16()
    # the style shifts: integer rows read through column slices; conv_k's row is centred at minus its
    # ROUTE_MEANS entry times the conv's folded scale, as a BatchNorm shift with that mean would be
    wide = _ri(g, -3, 3, N, 3 * C + 64)
    up = route_net().upsample.up[3]
    for k in (1, 2, 3):
        wide[:, 32 + (k - 1) * C: 32 + k * C] -= ROUTE_MEANS["up"][k] * bn64(up.conv[k].conv[0])[0].float()
    return SimpleNamespace(src=half(N, 2 * S, 2 * S, C // 2), xcur=half(N, S, S, C), y=half(N, S, S, C),
                           top_act=(_ri(g, 0, 6, N, S, S, C) / 2).bfloat16(), shifts_wide=wide,
                           shifts={(3, k): wide[:, 32 + (k - 1) * C: 32 + k * C] for k in (1, 2, 3)})


def down_model(net, src: torch.Tensor):
    """``resdown.forward`` of the deepest level on ``pool(src)``, as the engine stores it: the residual
    projection and every conv output rounded once, every activated copy twice.  -> (tensors, launches)."""
    blk, nxt = net.downsample.down[3], net.upsample.up[3].conv[0]
    s = src.double()
    q = [s[:, dy::2, dx::2] for dy in (0, 1) for dx in (0, 1)]
    x = torch.maximum(torch.maximum(q[0], q[1]), torch.maximum(q[2], q[3]))
    act = [bn64(blk.conv[k][0]) for k in range(4)] + [bn64(nxt[0])]
    L, T = {}, {}
    sp, tp = bn64(blk.proj[0])
    L["proj"] = launch64(_bf16_number(x * sp + tp, "the projection's input"), *_conv_of(blk.proj), name="down proj")
    T["proj"] = L["proj"].out
    a0 = _bf16_number((x * act[0][0] + act[0][1]).clamp_min(0.0), "c0's activated input")
    L["c0"] = launch64(a0, *_conv_of(blk.conv[0]), None, *act[1], name="down c0")
    T["ha"] = L["c0"].aout
    L["c1"] = launch64(T["ha"], *_conv_of(blk.conv[1]), T["proj"], *act[2], name="down c1")
    T["x1"], T["x1a"] = L["c1"].out, L["c1"].aout
    L["c2"] = launch64(T["x1a"], *_conv_of(blk.conv[2]), None, *act[3], name="down c2")
    T["h2a"] = L["c2"].aout
    L["c3"] = launch64(T["h2a"], *_conv_of(blk.conv[3]), T["x1"], *act[4], name="down c3")
    T["xd"], T["top_act"] = L["c3"].out, L["c3"].aout
    return T, L


def up_model(net, xcur, y, shifts: dict, top_act):
    """``resup.forward`` of the block at the deepest resolution.  ``top_act`` stands for conv_0's activated
    input and ``shifts[(3, k)]`` for conv_k's whole per-image shift ``full(style) * scale + shift``."""
    blk = net.upsample.up[3]
    sc = {k: bn64(blk.conv[k].conv[0])[0] for k in (1, 2, 3)}
    L, T = {}, {}
    sp, tp = bn64(blk.proj[0])
    L["proj"] = launch64(_bf16_number(xcur.double() * sp + tp, "the projection's input"), *_conv_of(blk.proj),
                         name="up proj")
    T["proj"] = L["proj"].out
    L["c0"] = launch64(top_act, *_conv_of(blk.conv[0]), y, sc[1], shifts[(3, 1)], name="up c0")
    T["h0a"] = L["c0"].aout
    L["c1"] = launch64(T["h0a"], *_conv_of(blk.conv[1].conv), T["proj"], sc[2], shifts[(3, 2)], name="up c1")
    T["x1"], T["x1a"] = L["c1"].out, L["c1"].aout
    L["c2"] = launch64(T["x1a"], *_conv_of(blk.conv[2].conv), None, sc[3], shifts[(3, 3)], name="up c2")
    T["h2a"] = L["c2"].aout
    L["c3"] = launch64(T["h2a"], *_conv_of(blk.conv[3].conv), T["x1"], name="up c3")
    T["out"] = L["c3"].out
    return T, L


@functools.lru_cache(maxsize=None)
def route_models():
    net, i = route_net(), route_inputs()
    return down_model(net, i.src), up_model(net, i.xcur, i.y, i.shifts, i.top_act)


if __name__ == "__main__":  # the figures of the module docstring
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for c in cases() + PP_EXTRA:
        s = check_exactness(data(c.name))
        print(f"{c.name:48s} out {100 * s['frac']:5.1f} %  2nd {100 * s['frac2']:5.1f} %  distinct {s['distinct']:5d}"
              f"  magnitude {s['mag']:.4f} of 2^22 q")
    for T, L in route_models():
        for k, m in L.items():
            r = (m.out.double() != m.yr).double().mean().item()
            print(f"route {k:5s} q 2^{int(torch.log2(torch.tensor(m.q)).item()):3d}  magnitude {m.mag:.3f} of 2^22 q"
                  f"  out rounded {100 * r:5.1f} %")
