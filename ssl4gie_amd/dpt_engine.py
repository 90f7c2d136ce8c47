"""Autograd nodes of the DPT dense decoder on the HIP engine.

Maps are channels-last ([B, H, W, C], the token-major layout of the ViT carried to the upsampled
resolutions) in the engine's operand type.  Every convolution runs on libssl4gie_hip.so:
  * Conv2d(k=1)            -> engine.LinearFn on [B*H*W, Cin]
  * ConvTranspose2d(k = s) -> GEMM against W[(i, j, co), ci] + pixel-shuffle scatter
  * Conv2d(k=3, pad=1)     -> Conv3x3Fn, every 3x3 layer of the package (ResNet-50 bottlenecks, this decoder, ConvStem,
                              FPN and RPN heads) on one of three kernel families: direct halo-in-LDS kernels, 256x256
                              GEMMs that gather the (dy, dx, ci) patch matrix in the kernel, plain GEMMs over a
                              materialised one (recomputed in backward: it is 9x the activation).  Which one the
                              forward, the weight gradient (bias gradient fused in) and the data gradient (flipped
                              kernel at stride 1, patch-matrix transpose at stride 2) take: conv_plan.conv3x3_plan.
Weight re-layouts (a few MB, once per optimizer step: LPCache.derived) and the scatter of dW back into the parameter's
[Cout, Cin, 3, 3] layout are small launches; all activation-sized work is HIP.  Reference: Models/DPT_decoder.py.
"""
from __future__ import annotations

import contextlib

import torch

from . import ops
from .conv_plan import conv3x3_plan
from .engine import GradSink, LPCache, wgrad_fork


def _operand(lp: LPCache, weight, dtype, mode, ld=None):
    """cached operand image ops.conv3x3_weight_pack(weight, dtype, mode, ld); ld None: unpadded rows, what the direct
    kernels read — for mode 0 that is the GEMM's image itself wherever its rows need no padding"""
    if ld is None and mode == 0 and ops.k_pad(9 * weight.shape[1], dtype) == 9 * weight.shape[1]:
        ld = 9 * weight.shape[1]
    tag = ("c3x", "c3dd")[mode] if ld is None else f"{('c3', 'c3d', 'c3t')[mode]}:{ld}"
    return lp.derived(weight, tag, dtype, lambda w: ops.conv3x3_weight_pack(w, dtype, mode, ld), recipe=(mode, ld))


def _pad_cols(m: torch.Tensor, ld: int) -> torch.Tensor:
    if m.shape[1] == ld:
        return m
    out = m.new_zeros(m.shape[0], ld)
    out[:, :m.shape[1]] = m
    return out


def _write_grad(target: torch.Tensor, value: torch.Tensor, accumulate: bool):
    if accumulate:
        target.add_(value)
    else:
        target.copy_(value)


class TokensToMapFn(torch.autograd.Function):
    """Slice(1) -> Transpose -> Unflatten (DPT_decoder.py:5-11, :328-332, :449-459): fp32 tap
    [B, 1+L, D] -> [B*L, D] operand rows (= the [B, 14, 14, D] map)."""

    @staticmethod
    def forward(ctx, z, dtype):
        ctx.shape = z.shape
        return ops.tokens_to_map(z.contiguous(), dtype)

    @staticmethod
    def backward(ctx, dx):
        B, L1, D = ctx.shape
        return ops.map_to_tokens(dx.contiguous(), B, L1 - 1, D), None


class Conv3x3Fn(torch.autograd.Function):
    """y = conv3x3(act(x)) + bias, pad 1, stride 1 or 2; act = ReLU if relu_in
    (layer*_rn :412-447, ResidualConvUnit_custom :212-233, output_conv.0/.2 :469-478,
    act_postprocess42.1 :397-403).  Kernels as conv_plan.conv3x3_plan says."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, relu_in, sink: GradSink, lp: LPCache, want_stats=False):
        """want_stats: also return BatchNorm partial statistics of y (see engine.LinearFn) or None"""
        B, H, W, Cin = x.shape
        Cout, dt = weight.shape[0], x.dtype
        plan = conv3x3_plan(B, H, W, Cin, Cout, stride, dt, bias is not None, bool(want_stats))
        w2 = _operand(lp, weight, dt, 0, plan.ld)
        x = x.contiguous()
        b = bias.detach() if bias is not None else None
        ctx.save_for_backward(x, weight, bias)
        ctx.cfg = (stride, relu_in, sink, lp, plan)
        if plan.fwd == "direct":
            out = ops.conv3x3_direct_fwd(x, _operand(lp, weight, dt, 0), b, relu_in, colstats=plan.fwd_stats)
        elif plan.fwd == "gather":  # patch matrix gathered in the GEMM
            out = ops.conv3x3_fwd(x, w2, b, stride, relu_in, colstats=plan.fwd_stats)
        else:
            out = ops.linear_fwd(ops.im2col3x3(x, stride, relu_in, plan.ld), w2, b, out_dtype=dt,
                                 colstats=plan.fwd_stats)
        y, stats = out if plan.fwd_stats else (out, None)
        if plan.fwd_stats:
            ctx.mark_non_differentiable(stats)
            ctx.set_materialize_grads(False)  # no zero tensor for the statistics' (absent) gradient
        if y.dim() == 2:  # the plain GEMM's [pixels, Cout]
            y = y.view(B, *ops.conv_out_hw(H, W, stride), Cout)
        return (y, stats) if want_stats else y

    @staticmethod
    def backward(ctx, dy, *unused):
        if dy is None:  # the map itself was not used downstream (gradients are not materialised)
            return (None,) * 8
        x, weight, bias = ctx.saved_tensors
        stride, relu_in, sink, lp, plan = ctx.cfg
        dy = dy.contiguous()
        (tw, tb), acc, rets = sink.plan([weight, bias])
        side = wgrad_fork(sink, (weight, bias), dy, x, weight, bias) if tw is not None else None
        with (torch.cuda.stream(side) if side is not None else contextlib.nullcontext()):
            Conv3x3Fn._wgrad(tw, tb, acc, dy.view(-1, weight.shape[0]), x, stride, relu_in, plan)
        dx = Conv3x3Fn._dgrad(dy, x, weight, stride, relu_in, lp, plan) if ctx.needs_input_grad[0] else None
        return dx, rets[0], rets[1], None, None, None, None, None

    @staticmethod
    def _wgrad(tw, tb, acc, dy2, x, stride, relu_in, plan):
        if tw is not None:
            Cout, Cin = tw.shape[:2]
            fuse_b = tb is not None and not acc  # the bias gradient rides on the same product
            bias_out = tb if fuse_b else None
            if plan.wgrad == "direct":
                dw2 = ops.conv3x3_direct_wgrad(dy2, x, relu_in, bias_out=bias_out)
            elif plan.wgrad == "gather":
                dw2 = ops.conv3x3_bwd_weight(dy2, x, stride, relu_in, bias_out=bias_out)
            else:
                dw2 = ops.linear_bwd_weight(dy2, ops.im2col3x3(x, stride, relu_in, plan.ld),  # recomputed, not kept
                                            bias_out=bias_out)
            if tb is not None and not fuse_b:
                ops.colsum(dy2, out=tb, accumulate=True)
            if dw2.dtype == torch.float32 and dw2.stride(1) == 1 and tw.is_contiguous():
                ops.conv3x3_wgrad_unpack(dw2, tw, acc)
            else:
                _write_grad(tw, dw2[:, :9 * Cin].view(Cout, 3, 3, Cin).permute(0, 3, 1, 2), acc)
        elif tb is not None:
            ops.colsum(dy2, out=tb, accumulate=acc)

    @staticmethod
    def _dgrad(dy, x, weight, stride, relu_in, lp, plan):
        B, H, W, Cin = x.shape
        Cout, dt = weight.shape[0], x.dtype
        if plan.dgrad == "col2im":
            w2, w2t = _operand(lp, weight, dt, 0, plan.ld), _operand(lp, weight, dt, 2, plan.ld)
            dcols = ops.linear_bwd_data(dy.view(-1, Cout), w2, w2t)  # [M_out, ld]
            dxr = ops.col2im3x3(dcols, B, H, W, Cin, stride)
        else:
            wd = _operand(lp, weight, dt, 1, plan.ld2)
            dy4 = dy.view(B, H, W, Cout)
            if plan.dgrad == "direct":  # the same direct kernel on dy with the flipped weight
                return ops.conv3x3_direct_fwd(dy4, _operand(lp, weight, dt, 1), None, relu_mask=x if relu_in else None)
            if plan.dgrad == "gather":  # the ReLU in front of this convolution masks its data gradient in the epilogue
                return ops.conv3x3_fwd(dy4, wd, None, 1, False, relu_mask=x if relu_in else None)
            dxr = ops.linear_fwd(ops.im2col3x3(dy4, 1, False, plan.ld2), wd, None, out_dtype=dt).view(B, H, W, Cin)
        return ops.relu_bwd(x, dxr) if relu_in else dxr


class ConvTransposeFn(torch.autograd.Function):
    """ConvTranspose2d(kernel = stride = k) on a [B*H*W, Cin] map (act_postprocess12.1 :345-354,
    act_postprocess22.1 :371-380): GEMM against W2[(i, j, co), ci] = weight[ci, co, i, j], then a
    pixel-shuffle scatter that also adds the bias."""

    @staticmethod
    def forward(ctx, x2, weight, bias, B, H, W, sink: GradSink, lp: LPCache):
        Cin, Cout, k, _ = weight.shape
        dt = x2.dtype
        ld = ops.k_pad(Cin, dt)
        if ld != Cin:
            # Cin = 96 (act_postprocess1) is not a whole number of the bf16 GEMM's 64-deep K-tiles: with
            # zero-padded operand copies (6 MB) the product runs on the MFMA bf16 kernel instead of the
            # generic fp32 one (164 -> ~20 us)
            w2 = lp.derived(weight, f"ct:{ld}", dt,
                          lambda w: _pad_cols(w.permute(2, 3, 1, 0).reshape(k * k * Cout, Cin), ld))
            g = ops.linear_fwd(_pad_cols(x2, ld), w2, None, out_dtype=dt)
        else:
            w2 = lp.derived(weight, "ct", dt, lambda w: w.permute(2, 3, 1, 0).reshape(k * k * Cout, Cin))
            g = ops.linear_fwd(x2, w2, None, out_dtype=dt)
        y = ops.pixel_shuffle(g, bias.detach(), B, H, W, k, Cout)
        ctx.save_for_backward(x2, weight, bias)
        ctx.cfg = (B, H, W, sink, lp)
        return y

    @staticmethod
    def backward(ctx, dy):
        x2, weight, bias = ctx.saved_tensors
        B, H, W, sink, lp = ctx.cfg
        Cin, Cout, k, _ = weight.shape
        dt = x2.dtype
        dy = dy.contiguous()
        dg = ops.pixel_unshuffle(dy, k)  # [B*H*W, k*k*Cout]
        (tw, tb), acc, rets = sink.plan([weight, bias])
        if tw is not None:
            dw2 = ops.linear_bwd_weight(dg, x2)  # [k*k*Cout, Cin]
            _write_grad(tw, dw2.view(k, k, Cout, Cin).permute(3, 2, 0, 1), acc)
        if tb is not None:
            ops.colsum(dy.view(-1, Cout), out=tb, accumulate=acc)
        dx = None
        if ctx.needs_input_grad[0]:
            w2 = lp.derived(weight, "ct", dt, lambda w: w.permute(2, 3, 1, 0).reshape(k * k * Cout, Cin))
            w2t = lp.derived(weight, "ct_t", dt,
                           lambda w: w.permute(2, 3, 1, 0).reshape(k * k * Cout, Cin).t())
            dx = ops.linear_bwd_data(dg, w2, w2t)
        return dx, rets[0], rets[1], None, None, None, None, None


class Upsample2xFn(torch.autograd.Function):
    """bilinear x2, align_corners=True (FeatureFusionBlock_custom.forward :293-295; Interpolate)."""

    @staticmethod
    def forward(ctx, x):
        return ops.bilinear2x_fwd(x.contiguous())

    @staticmethod
    def backward(ctx, dy):
        return ops.bilinear2x_bwd(dy.contiguous())


class ForkFn(torch.autograd.Function):
    """x -> (x, x) for a tensor with two consumers (the input of a residual unit feeds its first convolution AND
    its skip add, DPT_decoder.py:212-233): autograd would otherwise sum the two incoming gradients itself, with a
    torch clone + add kernel per fork (7 per depth step); here the sum is the library's element-wise kernel."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x), x.view_as(x)

    @staticmethod
    def backward(ctx, ga, gb):
        if ga is None or gb is None:
            return ga if gb is None else gb
        return ops.eltwise_add(ga.contiguous(), gb.contiguous())


class AddFn(torch.autograd.Function):
    """skip_add.add (:233, :290): FloatFunctional in float mode is a plain add."""

    @staticmethod
    def forward(ctx, a, b):
        return ops.eltwise_add(a.contiguous(), b.contiguous())

    @staticmethod
    def backward(ctx, g):
        return g, g


class DepthHeadFn(torch.autograd.Function):
    """ReLU -> Conv2d(32, 1, 1) -> Sigmoid (output_conv.3-.5, :479-481) -> fp32 [B, 1, H, W]."""

    @staticmethod
    def forward(ctx, x, weight, bias, sink: GradSink):
        B, H, W, C = x.shape
        x2 = x.contiguous().view(-1, C)
        w = weight.detach().reshape(-1).contiguous()
        y = ops.depth_head_fwd(x2, w, bias.detach())
        ctx.save_for_backward(x2, weight, bias, y)
        ctx.cfg = (B, H, W, sink)
        return y.view(B, 1, H, W)

    @staticmethod
    def backward(ctx, dy):
        x2, weight, bias, y = ctx.saved_tensors
        B, H, W, sink = ctx.cfg
        (tw, tb), acc, rets = sink.plan([weight, bias])
        dw = tw.view(-1) if tw is not None else torch.empty(weight.numel(), device=x2.device)
        db = tb if tb is not None else torch.empty(1, device=x2.device)
        dx = ops.depth_head_bwd(x2, weight.detach().reshape(-1).contiguous(), y,
                                dy.contiguous().view(-1).float(), dw, db, acc)
        return dx.view(B, H, W, -1), rets[0], rets[1], None


class SegHeadFn(torch.autograd.Function):
    """Conv2d(C, num_classes, 1) -> bilinear x2 (output_conv.4-.5 of the seg head, :483-497) ->
    fp32 logits [B, num_classes, 2H, 2W].  num_classes is tiny (1 for the binary task): the 1x1
    convolution runs as a GEMM against the weight padded to 8 output channels so that the map stays
    16-byte aligned through the bilinear kernel; the padding channels are dropped at the end."""

    @staticmethod
    def forward(ctx, x, weight, bias, sink: GradSink, lp: LPCache):
        B, H, W, C = x.shape
        nc = weight.shape[0]
        ncp = (nc + 7) // 8 * 8
        dt = x.dtype
        x2 = x.contiguous().view(-1, C)

        def pad_w(w):
            out = w.new_zeros(ncp, C)
            out[:nc] = w.reshape(nc, C)
            return out
        w8 = lp.derived(weight, f"seg:{ncp}", dt, pad_w)
        b8 = torch.zeros(ncp, dtype=torch.float32, device=x.device)
        b8[:nc] = bias.detach()
        y = ops.linear_fwd(x2, w8, b8, out_dtype=dt)
        up = ops.bilinear2x_fwd(y.view(B, H, W, ncp))
        ctx.save_for_backward(x2, weight, bias)
        ctx.cfg = (B, H, W, nc, ncp, sink, lp)
        return up[..., :nc].permute(0, 3, 1, 2).float().contiguous()

    @staticmethod
    def backward(ctx, dy):
        x2, weight, bias = ctx.saved_tensors
        B, H, W, nc, ncp, sink, lp = ctx.cfg
        C = x2.shape[1]
        dt = x2.dtype
        g = torch.zeros(B, 2 * H, 2 * W, ncp, dtype=dt, device=dy.device)
        g[..., :nc] = dy.permute(0, 2, 3, 1)
        dy8 = ops.bilinear2x_bwd(g).view(-1, ncp)
        (tw, tb), acc, rets = sink.plan([weight, bias])
        if tw is not None:
            db8 = torch.empty(ncp, dtype=torch.float32, device=dy.device)
            dw8 = ops.linear_bwd_weight(dy8, x2, bias_out=db8)
            _write_grad(tw, dw8[:nc].view_as(tw), acc)
            if tb is not None:
                _write_grad(tb, db8[:nc], acc)
        dx = None
        if ctx.needs_input_grad[0]:
            def pad_w(w):
                out = w.new_zeros(ncp, C)
                out[:nc] = w.reshape(nc, C)
                return out
            w8 = lp.derived(weight, f"seg:{ncp}", dt, pad_w)
            dx = ops.linear_bwd_data(dy8, w8).view(B, H, W, C)
        return dx, rets[0], rets[1], None, None
