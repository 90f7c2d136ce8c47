"""Autograd nodes of DeepLabV3+ on the HIP engine (csrc/atrous_ops.hip).

Channels-last maps in the engine's operand type, as everywhere in the package:
  * DilatedConv3x3Fn   Conv2d(k=3, stride 1, padding = dilation): the dilated patch matrix through the plain GEMMs, with
                       the operand images of the undilated convolution (dpt_engine._operand) — not a conv_plan path
  * DepthwiseConv3x3Fn the depthwise half of smp's SeparableConv2d; the data gradient is the same kernel with the
                       weight flipped, the weight gradient goes through the GradSink
  * PointwisePadFn     its pointwise half on a map with zero pad channels (304 -> 320: whole GEMM K-tiles)
  * UpsampleACFn       nn.UpsamplingBilinear2d(scale_factor=s)
  * ConcatFn           torch.cat along channels; a [B, C] operand is a 1x1 map up-sampled to the others' size
  * FanOutFn           a map with n consumers: the gradient sum is the library's element-wise kernel
  * SegHeadACFn        Conv2d(C, classes, 1) -> UpsamplingBilinear2d -> fp32 NCHW logits
Reference: segmentation_models_pytorch 0.3.2, decoders/deeplabv3/decoder.py and base/heads.py (not vendored).
"""
from __future__ import annotations

import contextlib

import torch

from . import ops
from .dpt_engine import _operand, _write_grad
from .engine import GradSink, LPCache, wgrad_fork


class DilatedConv3x3Fn(torch.autograd.Function):
    """y = conv3x3(x), stride 1, padding = dilation, no bias (ResNet layer4 at output stride 16)."""

    @staticmethod
    def forward(ctx, x, weight, dilation, sink: GradSink, lp: LPCache, want_stats=False):
        """want_stats: also return BatchNorm partial statistics of y (see engine.LinearFn) or None"""
        B, H, W, Cin = x.shape
        Cout, dt = weight.shape[0], x.dtype
        ld = ops.k_pad(9 * Cin, dt)
        x = x.contiguous()
        w2 = _operand(lp, weight, dt, 0, ld)
        ctx.save_for_backward(x, weight)
        ctx.cfg = (int(dilation), sink, lp, ld)
        cols = ops.im2col3x3_dil(x, dilation, ld)
        stats = None
        if want_stats and ops.colstats_ok(cols.shape[0], Cout, ld, dt):
            y, stats = ops.linear_fwd(cols, w2, None, out_dtype=dt, colstats=True)
            ctx.mark_non_differentiable(stats)
            ctx.set_materialize_grads(False)  # no zero tensor for the statistics' (absent) gradient
        else:
            y = DilatedConv3x3Fn._product(cols, w2, Cin)
        y = y.view(B, H, W, Cout)
        return (y, stats) if want_stats else y

    @staticmethod
    def _product(cols, w2, c_tap):
        """cols @ w2^T; in the fp32 parity mode tap by tap (ops.linear_fwd_kblocks): nine short rounding chains"""
        if cols.dtype == torch.float32 and cols.shape[1] == 9 * c_tap:
            return ops.linear_fwd_kblocks(cols, w2, c_tap)
        return ops.linear_fwd(cols, w2, None, out_dtype=cols.dtype)

    @staticmethod
    def backward(ctx, dy, *unused):
        if dy is None:  # the map itself was not used downstream (gradients are not materialised)
            return (None,) * 6
        x, weight = ctx.saved_tensors
        dil, sink, lp, ld = ctx.cfg
        B, H, W, Cin = x.shape
        Cout, dt = weight.shape[0], x.dtype
        dy = dy.contiguous()
        (tw,), acc, rets = sink.plan([weight])
        if tw is not None:
            side = wgrad_fork(sink, (weight,), dy, x, weight)
            with (torch.cuda.stream(side) if side is not None else contextlib.nullcontext()):
                dw2 = ops.linear_bwd_weight(dy.view(-1, Cout), ops.im2col3x3_dil(x, dil, ld))  # recomputed, not kept
                if tw.is_contiguous():
                    ops.conv3x3_wgrad_unpack(dw2, tw, acc)
                else:
                    _write_grad(tw, dw2[:, :9 * Cin].view(Cout, 3, 3, Cin).permute(0, 3, 1, 2), acc)
        dx = None
        if ctx.needs_input_grad[0]:  # the same dilated convolution of dy with the flipped kernel
            ld2 = ops.k_pad(9 * Cout, dt)
            wd = _operand(lp, weight, dt, 1, ld2)
            dx = DilatedConv3x3Fn._product(ops.im2col3x3_dil(dy.view(B, H, W, Cout), dil, ld2), wd,
                                           Cout).view(B, H, W, Cin)
        return dx, rets[0], None, None, None, None


def _pad2d(m: torch.Tensor, rows: int, cols: int) -> torch.Tensor:
    out = m.new_zeros(rows, cols)
    out[:m.shape[0], :m.shape[1]] = m
    return out


class DepthwiseConv3x3Fn(torch.autograd.Function):
    """y = Conv2d(C, C, 3, padding = dilation, groups = C, bias=False)(x); weight fp32 [C, 1, 3, 3].  A map that carries
    zero pad channels behind the C real ones (the decoder's 304-channel concatenation, padded to whole GEMM K-tiles) runs
    against the weight padded with zero filters (lp: the operand cache that keeps it); its gradient rows are dropped."""

    @staticmethod
    def _weight(weight, C, lp):
        if weight.shape[0] == C:
            return weight.detach().contiguous()
        return lp.derived(weight, f"dwpad:{C}", torch.float32, lambda w: _pad2d(w.reshape(w.shape[0], 9), C, 9))

    @staticmethod
    def forward(ctx, x, weight, dilation, sink: GradSink, lp: LPCache = None):
        x = x.contiguous()
        ctx.save_for_backward(x, weight)
        ctx.cfg = (int(dilation), sink, lp)
        return ops.dwconv3x3_fwd(x, DepthwiseConv3x3Fn._weight(weight, x.shape[-1], lp).view(-1, 1, 3, 3), dilation)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dil, sink, lp = ctx.cfg
        dy = dy.contiguous()
        (tw,), acc, rets = sink.plan([weight])
        if tw is not None:
            if tw.is_contiguous() and tw.shape[0] == x.shape[-1]:
                ops.dwconv3x3_wgrad(dy, x, dil, out=tw, accumulate=acc)  # straight into the gradient slice
            else:
                _write_grad(tw, ops.dwconv3x3_wgrad(dy, x, dil)[:tw.shape[0]], acc)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = ops.dwconv3x3_fwd(dy, DepthwiseConv3x3Fn._weight(weight, x.shape[-1], lp).view(-1, 1, 3, 3), dil, flip=True)
        return dx, rets[0], None, None, None


class PointwisePadFn(torch.autograd.Function):
    """Conv2d(K, N, 1, bias=False) on a map that carries Kp - K zero pad channels (K = 304 -> Kp = 320: whole 64-deep
    K-tiles, so the product runs on the bf16 MFMA kernels and can hand out BatchNorm statistics): the weight operand
    is padded with zero columns, as ConvTransposeFn pads its 96-channel input; the pad columns of dW are dropped."""

    @staticmethod
    def _operands(weight, Kp, dt, lp):
        N = weight.shape[0]
        w = lp.derived(weight, f"pw:{Kp}", dt, lambda w: _pad2d(w.reshape(N, -1), N, Kp))
        wt = lp.derived(weight, f"pwt:{Kp}", dt, lambda w: _pad2d(w.reshape(N, -1), N, Kp).t())
        return w, wt

    @staticmethod
    def forward(ctx, x, weight, sink: GradSink, lp: LPCache):
        """-> (y [..., N], BatchNorm partial statistics of y or None)"""
        shp, dt = x.shape, x.dtype
        x2 = x.contiguous().view(-1, shp[-1])
        w, _ = PointwisePadFn._operands(weight, shp[-1], dt, lp)
        ctx.save_for_backward(x2, weight)
        ctx.cfg = (shp, sink, lp)
        stats = None
        if ops.colstats_ok(x2.shape[0], w.shape[0], w.shape[1], dt):
            y, stats = ops.linear_fwd(x2, w, None, out_dtype=dt, colstats=True)
            ctx.mark_non_differentiable(stats)
            ctx.set_materialize_grads(False)  # no zero tensor for the statistics' (absent) gradient
        else:
            y = ops.linear_fwd(x2, w, None, out_dtype=dt)
        return y.view(*shp[:-1], w.shape[0]), stats

    @staticmethod
    def backward(ctx, dy, *unused):
        x2, weight = ctx.saved_tensors
        shp, sink, lp = ctx.cfg
        dy2 = dy.contiguous().view(-1, dy.shape[-1])
        (tw,), acc, rets = sink.plan([weight])
        dx = None
        if ctx.needs_input_grad[0]:
            w, wt = PointwisePadFn._operands(weight, shp[-1], x2.dtype, lp)
            dx = ops.linear_bwd_data(dy2, w, wt).view(shp)
        if tw is not None:
            dw = ops.linear_bwd_weight(dy2, x2)   # [N, Kp] fp32
            _write_grad(tw, dw[:, :tw.shape[1]].reshape(tw.shape), acc)
        return dx, rets[0], None, None


class UpsampleACFn(torch.autograd.Function):
    """nn.UpsamplingBilinear2d(scale_factor=scale): bilinear, align_corners=True."""

    @staticmethod
    def forward(ctx, x, scale):
        ctx.scale = int(scale)
        return ops.bilinear_up_ac_fwd(x.contiguous(), scale)

    @staticmethod
    def backward(ctx, dy):
        return ops.bilinear_up_ac_bwd(dy.contiguous(), ctx.scale), None


class ConcatFn(torch.autograd.Function):
    """torch.cat(parts, dim=channels) -> one [B, H, W, sum C] buffer, every part written into its channel slice.  A
    [B, C] part stands for a 1x1 map up-sampled to H x W (ASPPPooling: F.interpolate of a single pixel is a constant),
    so its gradient is the per-image sum over the pixels of its slice."""

    @staticmethod
    def forward(ctx, *parts):
        ref = next(p for p in parts if p.dim() == 4)
        B, H, W, _ = ref.shape
        widths = [p.shape[-1] for p in parts]
        out = torch.empty(B, H, W, sum(widths), dtype=ref.dtype, device=ref.device)
        off = 0
        for p, c in zip(parts, widths):
            ops.chan_write(out, off, p.contiguous())
            off += c
        ctx.cfg = (widths, [p.dim() for p in parts], H * W)
        return out

    @staticmethod
    def backward(ctx, g):
        widths, dims, hw = ctx.cfg
        g = g.contiguous()
        grads, off = [], 0
        for i, (c, nd) in enumerate(zip(widths, dims)):
            gi = None
            if ctx.needs_input_grad[i]:
                gi = ops.chan_read(g, off, c)
                if nd == 2:  # [B, C] floats: the pixel mean of the slice times the pixel count
                    gi = (ops.avgpool_fwd(gi) * float(hw)).to(g.dtype)
            grads.append(gi)
            off += c
        return tuple(grads)


class FanOutFn(torch.autograd.Function):
    """x -> n views of x for a map with n consumers (the layer4 map feeds the five ASPP branches): the incoming
    gradients are summed by the library's element-wise kernel, in branch order."""

    @staticmethod
    def forward(ctx, x, n):
        return tuple(x.view_as(x) for _ in range(n))

    @staticmethod
    def backward(ctx, *gs):
        total = None
        for g in gs:
            if g is not None:
                total = g.contiguous() if total is None else ops.eltwise_add(total, g.contiguous())
        return total, None


class SegHeadACFn(torch.autograd.Function):
    """smp SegmentationHead: Conv2d(C, classes, 1) -> UpsamplingBilinear2d(scale) -> fp32 logits [B, classes, sH, sW].
    `classes` is tiny: the 1x1 convolution is a GEMM against the weight padded with zero rows to 8 output columns
    (as dpt_engine.SegHeadFn pads it), written in fp32; only the real columns are up-sampled."""

    @staticmethod
    def _pad_w(nc, ncp, C):
        def pad(w):
            out = w.new_zeros(ncp, C)
            out[:nc] = w.reshape(nc, C)
            return out
        return pad

    @staticmethod
    def forward(ctx, x, weight, bias, scale, sink: GradSink, lp: LPCache):
        B, H, W, C = x.shape
        nc = weight.shape[0]
        ncp = (nc + 7) // 8 * 8
        dt = x.dtype
        x2 = x.contiguous().view(-1, C)
        w8 = lp.derived(weight, f"segac:{ncp}", dt, SegHeadACFn._pad_w(nc, ncp, C))
        b8 = torch.zeros(ncp, dtype=torch.float32, device=x.device)
        b8[:nc] = bias.detach()
        y = ops.linear_fwd(x2, w8, b8, out_dtype=torch.float32).view(B, H, W, ncp)
        y = ops.chan_read(y, 0, nc)
        up = ops.bilinear_up_ac_fwd(y, scale) if scale > 1 else y
        ctx.save_for_backward(x2, weight, bias)
        ctx.cfg = (B, H, W, nc, ncp, int(scale), sink, lp)
        return up.view(B, 1, *up.shape[1:3]) if nc == 1 else up.permute(0, 3, 1, 2).contiguous()

    @staticmethod
    def backward(ctx, dy):
        x2, weight, bias = ctx.saved_tensors
        B, H, W, nc, ncp, scale, sink, lp = ctx.cfg
        C, dt = x2.shape[1], x2.dtype
        dy = dy.float()
        g = dy.contiguous().view(B, dy.shape[2], dy.shape[3], 1) if nc == 1 else dy.permute(0, 2, 3, 1).contiguous()
        if scale > 1:
            g = ops.bilinear_up_ac_bwd(g, scale)
        if dt != torch.float32:
            g = ops.cast(g, dt)
        dy8 = torch.zeros(B, H, W, ncp, dtype=dt, device=g.device)
        ops.chan_write(dy8, 0, g)
        dy8 = dy8.view(-1, ncp)
        (tw, tb), acc, rets = sink.plan([weight, bias])
        if tw is not None:
            db8 = torch.empty(ncp, dtype=torch.float32, device=g.device)
            dw8 = ops.linear_bwd_weight(dy8, x2, bias_out=db8)
            _write_grad(tw, dw8[:nc].view_as(tw), acc)
            if tb is not None:
                _write_grad(tb, db8[:nc], acc)
        dx = None
        if ctx.needs_input_grad[0]:
            w8 = lp.derived(weight, f"segac:{ncp}", dt, SegHeadACFn._pad_w(nc, ncp, C))
            dx = ops.linear_bwd_data(dy8, w8).view(B, H, W, C)
        return dx, rets[0], rets[1], None, None, None
