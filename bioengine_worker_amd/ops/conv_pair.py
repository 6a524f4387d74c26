"""Fused residual half-block: two pre-activation 3x3 convs, intermediate kept in LDS
(HIP kernel ``csrc/kernels/conv_pair.hip``).

``conv_pair`` computes::

    h   = relu( (convA(actA(inxform(x))) + biasA [+ x2]) * sB + tB )
    out = convB(h) + biasB [+ convP(actP(x)) + biasP] [+ res | + up2(res)]

with ``actA(v) = relu(v * sA + tA)``, ``actP(v) = v * sP + tP``.  ``tA``/``tB`` may be per-image
``[N, C]`` rows (the folded style vector of cellpose ``batchconvstyle``).  Two calls make one Cellpose
CPnet residual block (``resdown``/``resup``, reached by the reference through
cellpose==3.1.1.2, ``/root/reference/apps/model-runner/runtime_deployment.py:19``).

The kernel never writes ``h`` to HBM; it rounds it to bf16 ONCE after actB (the per-layer path
rounds the raw conv output and then the activation), so :func:`conv_pair_ref` mirrors exactly that.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch
import torch.nn.functional as F

from . import _native
from .conv import INMODES, PackedConv, _act_ref, _affine_stride, fused_conv2d, fused_conv2d_ref, out_hw

#: (Cin, CM, inmode, x2, proj, res) combinations the kernel is instantiated for (CPnet levels 0/1)
SUPPORTED = {
    (8, 32, "none", False, True, "none"),
    (32, 32, "none", False, False, "full"),
    (64, 32, "up2", True, False, "up2"),
    (32, 64, "pool2", False, False, "full"),
    (64, 64, "none", False, False, "full"),
    (128, 64, "up2", True, False, "up2"),
}
RESMODES = {"none": 0, "full": 1, "up2": 2}
#: configurations with a CM = 64 ping-pong build (``conv_pair_pp64.inc``): these calls also pass the
#: weights in MFMA-fragment order (:func:`pack_frag`)
FRAG_CONFIGS = {
    (64, 64, "none", False, False, "full"),
    (32, 64, "pool2", False, False, "full"),
    (128, 64, "up2", True, False, "up2"),
}
#: configurations whose projection is ROUNDED to bf16 before it is added (``PairSpec.bias_p`` apart
#: from ``bias``): the result of the per-layer 1x1 projection followed by the pair with that tensor
#: as its residual, which is also how they run (two launches) unless the native side takes the call
#: on the ping-pong build with the projection inside (``be_conv_pair_proj``)
PROJ_CONFIGS = {
    (32, 64, "pool2", False, True, "none"),
}
SUPPORTED |= PROJ_CONFIGS


def pack_proj_frag(wp: torch.Tensor) -> torch.Tensor:
    """A 1x1 projection's ``PackedConv.wp`` ``[64, 1, 32]`` in MFMA-A-fragment order
    ``[1, 4 channel tiles, 64 lanes, 8]``: lane ``kq * 16 + lrow`` of channel tile ``ct`` holds
    ``wp[ct * 16 + lrow, 0, kq * 8 : kq * 8 + 8]`` (one K-step of :func:`pack_frag`'s layout)."""
    cout, nchunk, kp = wp.shape
    assert cout == 64 and nchunk == 1 and kp == 32, "projection fragments: 32 -> 64 channels, 1x1"
    t = wp.reshape(4, 16, 4, 8)                      # ct, lrow, kq, e
    return t.permute(0, 2, 1, 3).contiguous().reshape(1, 4, 64, 8)


def unpack_proj_frag(wf: torch.Tensor) -> torch.Tensor:
    """Inverse of :func:`pack_proj_frag`."""
    return wf.reshape(4, 4, 16, 8).permute(0, 2, 1, 3).contiguous().reshape(64, 1, 32)


def pack_frag(wp: torch.Tensor) -> torch.Tensor:
    """``PackedConv.wp`` ``[64, nchunk, 288]`` (K index = tap * 32 + c) in MFMA-A-fragment order
    ``[nchunk, 9 taps, 4 channel tiles, 64 lanes, 8]``: lane ``kq * 16 + lrow`` of channel tile ``ct``
    holds ``wp[ct * 16 + lrow, chunk, tap * 32 + kq * 8 : ... + 8]``, the operand registers of one
    ``v_mfma_f32_16x16x32_bf16``, so a wave fetches a fragment with one 16-byte-per-lane load."""
    cout, nchunk, kp = wp.shape
    assert cout == 64 and kp == 288, "fragment packing: 64 output channels, 3x3 taps of 32-channel chunks"
    t = wp.reshape(4, 16, nchunk, 9, 4, 8)          # ct, lrow, chunk, tap, kq, e
    return t.permute(2, 3, 0, 4, 1, 5).contiguous().reshape(nchunk, 9, 4, 64, 8)


def unpack_frag(wf: torch.Tensor) -> torch.Tensor:
    """Inverse of :func:`pack_frag`."""
    nchunk = wf.shape[0]
    t = wf.reshape(nchunk, 9, 4, 4, 16, 8)          # chunk, tap, ct, kq, lrow, e
    return t.permute(2, 4, 0, 1, 3, 5).contiguous().reshape(64, nchunk, 288)


@dataclass
class PairSpec:
    """Weights + folded affines of one fused half-block.

    ``tb`` is actB's shift with convA's bias folded in (``tB + sB * biasA``) when it is shared; for a
    per-image shift the caller folds it into the style GEMM constants instead (``tb`` then None).
    ``bias`` is convB's bias plus the projection's bias, except in ``PROJ_CONFIGS``, where the
    projection is rounded to bf16 on its own and keeps its bias in ``bias_p``."""

    pa: PackedConv
    pb: PackedConv
    sa: torch.Tensor
    ta: torch.Tensor | None
    sb: torch.Tensor
    tb: torch.Tensor | None
    bias: torch.Tensor
    inmode: str = "none"
    pp: PackedConv | None = None
    sp: torch.Tensor | None = None
    tp: torch.Tensor | None = None
    #: fragment-order copies of ``pa.wp`` / ``pb.wp`` per device, built on first use (:meth:`frag`)
    frag_cache: dict | None = None
    #: ``PROJ_CONFIGS`` only: the projection's bias [CM] (zeros without one), NOT folded into ``bias``
    bias_p: torch.Tensor | None = None
    proj_frag_cache: dict | None = None
    plain: "PairSpec | None" = None

    def proj_rounded(self, has_x2: bool, res: str) -> bool:
        """The call is one of ``PROJ_CONFIGS``: projection rounded to bf16, its bias in ``bias_p``."""
        return self.bias_p is not None and (self.cin, self.cm, self.inmode, has_x2, self.pp is not None, res) in PROJ_CONFIGS

    def frag_proj(self, device: torch.device) -> torch.Tensor:
        """``pack_proj_frag(pp.wp)`` on ``device``; packed once and kept with the spec, as :meth:`frag`."""
        key = (str(device), self.pp.wp.data_ptr())
        if self.proj_frag_cache is None or self.proj_frag_cache.get("key") != key:
            self.proj_frag_cache = {"key": key, "w": pack_proj_frag(self.pp.wp.to(device))}
        return self.proj_frag_cache["w"]

    def frag(self, device: torch.device) -> tuple[torch.Tensor, torch.Tensor]:
        """``(pack_frag(pa.wp), pack_frag(pb.wp))`` on ``device``; packed once and kept with the spec
        (repacked if the packed weights were replaced)."""
        key = (str(device), self.pa.wp.data_ptr(), self.pb.wp.data_ptr())
        if self.frag_cache is None:
            self.frag_cache = {}
        if self.frag_cache.get("key") != key:  # updated in place: without_proj() shares the dict
            self.frag_cache.update(key=key, w=(pack_frag(self.pa.wp.to(device)), pack_frag(self.pb.wp.to(device))))
        return self.frag_cache["w"]

    @property
    def cm(self) -> int:
        return self.pb.cout

    @property
    def cin(self) -> int:
        return self.pa.cin_pad

    def supports(self, has_x2: bool, res: str) -> bool:
        cfg = (self.cin, self.cm, self.inmode, has_x2, self.pp is not None, res)
        return cfg in SUPPORTED and (cfg in PROJ_CONFIGS) == (self.bias_p is not None)

    def without_proj(self) -> "PairSpec":
        """The same half-block taking its projection as a residual: shares every tensor, made once (its
        fragment cache is this spec's, so neither route packs twice)."""
        if self.frag_cache is None:
            self.frag_cache = {}
        if self.plain is None:
            self.plain = PairSpec(pa=self.pa, pb=self.pb, sa=self.sa, ta=self.ta, sb=self.sb, tb=self.tb,
                                  bias=self.bias, inmode=self.inmode, frag_cache=self.frag_cache)
        return self.plain


def fold_bias(shift: torch.Tensor, scale: torch.Tensor, bias: torch.Tensor | None) -> torch.Tensor:
    """``t + s * b``: a conv bias pushed through the next pre-activation affine."""
    if bias is None:
        return shift.clone()
    n = bias.numel()
    out = shift.clone()
    out[..., :n] = out[..., :n] + scale[:n] * bias.to(shift.device)
    return out


def conv_pair_ref(x, spec: PairSpec, *, ta=None, tb=None, x2=None, res=None, res_mode="none"):
    """fp32 PyTorch oracle with the kernel's two bf16 rounding points (activated input, h)."""
    ta = spec.ta if ta is None else ta
    tb = spec.tb if tb is None else tb
    if spec.proj_rounded(x2 is not None, "none" if res is None else res_mode):
        # the composition of the two existing references: the per-layer projection, then the pair
        proj = fused_conv2d_ref(x, spec.pp, scale=spec.sp, shift=spec.tp, inmode=spec.inmode)
        return conv_pair_ref(x, spec.without_proj(), ta=ta, tb=tb, res=proj, res_mode="full")
    xf = x.float()
    a = _act_ref(xf, None, spec.sa, ta, True, spec.inmode).to(torch.bfloat16).float()
    wa = spec.pa.w.to(a.device)
    if wa.shape[1] < a.shape[1]:
        wa = F.pad(wa, (0, 0, 0, 0, 0, a.shape[1] - wa.shape[1]))
    hA = F.conv2d(a, wa.to(torch.bfloat16).float(), None, padding=1)
    if x2 is not None:
        hA = hA + x2.float().permute(0, 3, 1, 2)
    C = hA.shape[1]
    sb = spec.sb[:C].view(1, C, 1, 1)
    tbv = tb.view(-1, tb.shape[-1], 1, 1)[:, :C] if tb.dim() == 2 else tb[:C].view(1, C, 1, 1)
    h = torch.relu(hA * sb + tbv).to(torch.bfloat16).float()
    y = F.conv2d(h, spec.pb.w.to(h.device).to(torch.bfloat16).float(), None, padding=1)
    if spec.pp is not None:
        p = _act_ref(xf, None, spec.sp, spec.tp, False, spec.inmode).to(torch.bfloat16).float()
        wp = spec.pp.w.to(p.device)
        if wp.shape[1] < p.shape[1]:
            wp = F.pad(wp, (0, 0, 0, 0, 0, p.shape[1] - wp.shape[1]))
        y = y + F.conv2d(p, wp.to(torch.bfloat16).float(), None)
    y = y + spec.bias.to(y.device).view(1, -1, 1, 1)
    y = y.permute(0, 2, 3, 1)
    if res is not None:
        r = res.float()
        if res_mode == "up2":
            r = r.repeat_interleave(2, 1).repeat_interleave(2, 2)
        y = y + r
    return y.to(x.dtype).contiguous()


def conv_pair(x: torch.Tensor, spec: PairSpec, *, ta=None, tb=None, x2=None, res=None, res_mode: str = "none",
              out: torch.Tensor | None = None) -> torch.Tensor:
    """Run the fused half-block on NHWC bf16 ``x`` [N, Hs, Ws, Cin]; returns [N, H, W, CM] bf16.
    ``ta``/``tb`` override the spec's shifts (per-image [N, C] rows, convA bias already folded into
    ``tb``); ``res_mode`` is "full" (``res`` at output resolution) or "up2" (``res`` at half)."""
    ta = spec.ta if ta is None else ta
    tb = spec.tb if tb is None else tb
    assert ta is not None and tb is not None, "conv_pair needs actA / actB shifts"
    if res is None:
        res_mode = "none"
    if not x.is_cuda:
        y = conv_pair_ref(x, spec, ta=ta, tb=tb, x2=x2, res=res, res_mode=res_mode)
        if out is not None:
            out.copy_(y)
            return out
        return y
    N, Hs, Ws, Cin = x.shape
    H, W = out_hw(x, spec.inmode)
    CM = spec.cm
    assert x.dtype == torch.bfloat16 and x.is_contiguous(), "conv_pair expects contiguous NHWC bf16"
    assert Cin == spec.cin, f"input channels {Cin} != packed {spec.cin}"
    if spec.proj_rounded(x2 is not None, res_mode):
        return _conv_pair_proj(x, spec, ta, tb, out)
    if not spec.supports(x2 is not None, res_mode):
        raise ValueError(f"conv_pair: unsupported configuration {(Cin, CM, spec.inmode, x2 is not None, spec.pp is not None, res_mode)}")
    if x2 is not None:
        assert x2.shape == (N, H, W, CM) and x2.dtype == torch.bfloat16 and x2.is_contiguous()
    if res_mode == "full":
        assert res.shape == (N, H, W, CM) and res.dtype == torch.bfloat16 and res.is_contiguous()
    elif res_mode == "up2":
        assert res.shape == (N, H // 2, W // 2, CM) and res.dtype == torch.bfloat16 and res.is_contiguous()
    if out is None:
        out = torch.empty(N, H, W, CM, device=x.device, dtype=torch.bfloat16)
    else:
        assert out.shape == (N, H, W, CM) and out.dtype == torch.bfloat16 and out.is_contiguous()
        assert out.data_ptr() != x.data_ptr(), "conv_pair cannot run in place"
    ta_ns = _affine_stride(ta, N, Cin)
    tb_ns = _affine_stride(tb, N, CM)
    pp = spec.pp
    waf = wbf = None
    if (Cin, CM, spec.inmode, x2 is not None, pp is not None, res_mode) in FRAG_CONFIGS:
        waf, wbf = spec.frag(x.device)
    _native.call(
        "be_conv_pair_frag",
        _native.ptr(x), _native.ptr(x2), _native.ptr(spec.sa), _native.ptr(ta), ta_ns, _native.ptr(spec.sb),
        _native.ptr(tb), tb_ns, _native.ptr(spec.sp), _native.ptr(spec.tp), _native.ptr(spec.pa.wp),
        _native.ptr(spec.pb.wp), _native.ptr(None if pp is None else pp.wp), _native.ptr(spec.bias),
        _native.ptr(res), _native.ptr(out), N, H, W, Hs, Ws, Cin, CM, INMODES[spec.inmode], int(pp is not None),
        RESMODES[res_mode], _native.ptr(waf), _native.ptr(wbf), _native.stream(x.device),
    )
    return out


def proj_fused(x: torch.Tensor, spec: PairSpec) -> bool:
    """Whether a ``PROJ_CONFIGS`` call on ``x`` runs as ONE launch with the projection inside the
    ping-pong kernel.  The native side decides (``be_conv_pair_proj_takes``: the ping-pong kernel's own
    size rule, ``BE_PAIR_PP64``, the forced grid and the fusion's switch ``BE_PAIR_PP64_PROJ``)
    before anything is launched."""
    H, W = out_hw(x, spec.inmode)
    return x.is_cuda and bool(_native.hip().be_conv_pair_proj_takes(x.shape[0], H, W))


def _conv_pair_proj(x, spec: PairSpec, ta, tb, out):
    N, Hs, Ws, Cin = x.shape
    H, W = out_hw(x, spec.inmode)
    if not proj_fused(x, spec):
        # small calls (batch-1 latency, default-grid tests): the per-layer projection, then the pair
        proj = fused_conv2d(x, spec.pp, scale=spec.sp, shift=spec.tp, inmode=spec.inmode)
        return conv_pair(x, spec.without_proj(), ta=ta, tb=tb, res=proj, res_mode="full", out=out)
    CM = spec.cm
    if out is None:
        out = torch.empty(N, H, W, CM, device=x.device, dtype=torch.bfloat16)
    else:
        assert out.shape == (N, H, W, CM) and out.dtype == torch.bfloat16 and out.is_contiguous()
        assert out.data_ptr() != x.data_ptr(), "conv_pair cannot run in place"
    waf, wbf = spec.frag(x.device)
    _native.call(
        "be_conv_pair_proj",
        _native.ptr(x), _native.ptr(spec.sa), _native.ptr(ta), _affine_stride(ta, N, Cin), _native.ptr(spec.sb),
        _native.ptr(tb), _affine_stride(tb, N, CM), _native.ptr(spec.sp), _native.ptr(spec.tp), _native.ptr(spec.pa.wp),
        _native.ptr(spec.pb.wp), _native.ptr(spec.bias), _native.ptr(spec.bias_p), _native.ptr(out), N, H, W, Hs, Ws,
        Cin, CM, _native.ptr(waf), _native.ptr(wbf), _native.ptr(spec.frag_proj(x.device)), _native.stream(x.device),
    )
    return out


@dataclass
class HeadSpec:
    """The network's output layer (``relu(v * s + t)`` then a 1x1 conv with bias; eval BN folded)
    fused into the epilogue of the final 32-channel half-block (kernel ``be_conv_pair_head``).
    ``wh``: bf16 [16, 32], rows = output channels (zero past ``nh``), k axis permuted to the
    accumulator layout (lane group kq holds channels 4kq..4kq+3 and 16+4kq..16+4kq+3)."""

    s: torch.Tensor
    t: torch.Tensor
    w: torch.Tensor      # fp32 [nh, 32] original weights (reference path)
    b: torch.Tensor      # fp32 [16] bias, zero padded
    nh: int
    wh: torch.Tensor | None = None

    @staticmethod
    def k_order() -> list[int]:
        return [(kq * 4 + j) if j < 4 else (16 + kq * 4 + j - 4) for kq in range(4) for j in range(8)]

    @classmethod
    def build(cls, scale: torch.Tensor, shift: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None):
        nh, cin = weight.shape[0], weight.shape[1]
        assert cin <= 32 and nh <= 16 and weight.shape[2:] == (1, 1)
        dev = weight.device
        w = torch.zeros(nh, 32, device=dev)
        w[:, :cin] = weight.detach().float().reshape(nh, cin)
        b = torch.zeros(16, device=dev)
        if bias is not None:
            b[:nh] = bias.detach().float()
        s = torch.zeros(32, device=dev)
        t = torch.zeros(32, device=dev)
        s[: scale.numel()] = scale.float()
        t[: shift.numel()] = shift.float()
        wp = torch.zeros(16, 32, device=dev)
        wp[:nh] = w[:, cls.k_order()]
        return cls(s=s.contiguous(), t=t.contiguous(), w=w, b=b.contiguous(), nh=nh,
                   wh=wp.to(torch.bfloat16).contiguous())


def head_ref(xout: torch.Tensor, head: HeadSpec) -> torch.Tensor:
    """fp32 oracle of the fused head from the block output ``xout`` (NHWC bf16): the activated input is
    rounded to bf16 as the kernel's MFMA operand is."""
    a = torch.relu(xout.float() * head.s.to(xout.device) + head.t.to(xout.device))
    w = head.w.to(a.device)
    if xout.dtype == torch.bfloat16:  # the GPU path's rounding points (CPU fp32 runs stay fp32)
        a = a.to(torch.bfloat16).float()
        w = w.to(torch.bfloat16).float()
    y = torch.einsum("nhwc,oc->nohw", a, w) + head.b[: head.nh].to(a.device).view(1, -1, 1, 1)
    return y.contiguous()


def conv_pair_head(x: torch.Tensor, spec: PairSpec, head: HeadSpec, *, ta=None, tb=None, res=None) -> torch.Tensor:
    """Final up half-block (32 -> 32 channels, ``+ res`` at full resolution) with the output layer fused:
    returns fp32 NCHW [N, nh, H, W]; the block's own 32-channel output never reaches HBM."""
    ta = spec.ta if ta is None else ta
    tb = spec.tb if tb is None else tb
    assert ta is not None and tb is not None and res is not None
    if not x.is_cuda:
        return head_ref(conv_pair_ref(x, spec, ta=ta, tb=tb, res=res, res_mode="full"), head)
    N, H, W, Cin = x.shape
    assert spec.cin == 32 and spec.cm == 32 and spec.inmode == "none" and spec.pp is None, "head fusion: 32->32 only"
    assert x.dtype == torch.bfloat16 and x.is_contiguous() and Cin == 32
    assert res.shape == (N, H, W, 32) and res.dtype == torch.bfloat16 and res.is_contiguous()
    hout = torch.empty(N, head.nh, H, W, device=x.device, dtype=torch.float32)
    _native.call(
        "be_conv_pair_head",
        _native.ptr(x), _native.ptr(spec.sa), _native.ptr(ta), _affine_stride(ta, N, Cin), _native.ptr(spec.sb),
        _native.ptr(tb), _affine_stride(tb, N, 32), _native.ptr(spec.pa.wp), _native.ptr(spec.pb.wp),
        _native.ptr(spec.bias), _native.ptr(res), _native.ptr(head.s), _native.ptr(head.t), _native.ptr(head.wh),
        _native.ptr(head.b), _native.ptr(hout), head.nh, N, H, W, _native.stream(x.device),
    )
    return hout
