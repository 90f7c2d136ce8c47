"""Loss functions of the finetune heads.  BASELINE.json's north_star leaves loss reductions host-side
("Host code stays Python on PyTorch-ROCm for the DataLoader, optimizer step and loss reductions"):
the torch formulations below are that path, and the parity reference.  On the HIP device the two
module classes run fused device kernels instead (csrc/loss_ops.hip — value and
gradient in five / three launches instead of ~100 small ones); SSL4GIE_FUSED_LOSS=0 or CPU tensors
select the torch formulation.  The same file holds the loss heads of the other workloads: `SoftTargetCrossEntropy` /
`LabelSmoothingCrossEntropy` (the MAE fine-tuning recipe, `Models/mae/main_finetune.py:292-294`), `CrossEntropyLoss`
(the classification finetune's weighted cross-entropy, `Classification/train_classification.py:278`) and
`info_nce` (MoCo-v3's contrastive loss, `Models/moco_v3/moco/builder.py:63-73`).  Same call signature and numerics as the reference's
`Depth_estimation/Metrics/losses.py` (scale-and-shift-invariant depth loss, :120-146): per-image
closed-form 2x2 least squares for (scale, shift) on the valid pixels (:5-25), masked MSE / (2M)
(:51-57) and alpha x a 4-scale masked gradient L1 (:60-77, :104-117), batch-based reduction
(:28-38).  Written without the reference's data-dependent `nonzero()` indexing, so a step has no
device -> host synchronisation; results are identical (images with a singular system get
scale = shift = 0, an empty mask contributes 0).
"""
from __future__ import annotations

import torch
import torch.nn as nn


def compute_scale_and_shift(prediction, target, mask):
    mask = mask.to(prediction.dtype)
    a_00 = torch.sum(mask * prediction * prediction, (1, 2))
    a_01 = torch.sum(mask * prediction, (1, 2))
    a_11 = torch.sum(mask, (1, 2))
    b_0 = torch.sum(mask * prediction * target, (1, 2))
    b_1 = torch.sum(mask * target, (1, 2))
    det = a_00 * a_11 - a_01 * a_01
    ok = det != 0
    safe = torch.where(ok, det, torch.ones_like(det))
    x_0 = torch.where(ok, (a_11 * b_0 - a_01 * b_1) / safe, torch.zeros_like(det))
    x_1 = torch.where(ok, (-a_01 * b_0 + a_00 * b_1) / safe, torch.zeros_like(det))
    return x_0, x_1


def _batch_based(image_loss, M):
    divisor = torch.sum(M)
    total = torch.sum(image_loss)
    return torch.where(divisor == 0, torch.zeros_like(total), total / torch.clamp(divisor, min=1e-30))


def mse_loss(prediction, target, mask):
    mask = mask.to(prediction.dtype)
    M = torch.sum(mask, (1, 2))
    res = prediction - target
    return _batch_based(torch.sum(mask * res * res, (1, 2)), 2 * M)


def gradient_loss(prediction, target, mask):
    mask = mask.to(prediction.dtype)
    M = torch.sum(mask, (1, 2))
    diff = mask * (prediction - target)
    grad_x = torch.abs(diff[:, :, 1:] - diff[:, :, :-1]) * (mask[:, :, 1:] * mask[:, :, :-1])
    grad_y = torch.abs(diff[:, 1:, :] - diff[:, :-1, :]) * (mask[:, 1:, :] * mask[:, :-1, :])
    return _batch_based(torch.sum(grad_x, (1, 2)) + torch.sum(grad_y, (1, 2)), M)


def _fused_ok(*ts):
    import os
    return all(t.is_cuda for t in ts) and os.environ.get("SSL4GIE_FUSED_LOSS", "1") != "0"


class _SsiFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, prediction, target, alpha, scales):
        import ctypes  # noqa: F401
        from . import _lib
        from .ops import ptr, stream
        L = _lib.load()
        p = prediction.contiguous().float()
        t = target.contiguous().float()
        B, H, W = p.shape
        nb = L.ssl4gie_ssi_loss_workspace_bytes(B, H, W)
        ws = torch.empty(nb, dtype=torch.uint8, device=p.device)
        loss = torch.empty((), dtype=torch.float32, device=p.device)
        dpred = torch.empty_like(p)
        _lib.check(L.ssl4gie_ssi_loss(ptr(p), ptr(t), ptr(loss), ptr(dpred), B, H, W, float(alpha), int(scales),
                                      ptr(ws), stream()), "ssi_loss")
        ctx.save_for_backward(dpred)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dpred,) = ctx.saved_tensors
        return dpred * g, None, None, None


class _DiceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, targets, smooth):
        from . import _lib
        from .ops import ptr, stream
        L = _lib.load()
        B = logits.shape[0]
        l = logits.contiguous().float().view(B, -1)
        t = targets.contiguous().float().view(B, -1)
        ws = torch.empty(L.ssl4gie_dice_loss_workspace_bytes(B), dtype=torch.uint8, device=l.device)
        loss = torch.empty((), dtype=torch.float32, device=l.device)
        dl = torch.empty_like(l)
        _lib.check(L.ssl4gie_dice_loss(ptr(l), ptr(t), ptr(loss), ptr(dl), B, l.shape[1], float(smooth), ptr(ws),
                                       stream()), "dice_loss")
        ctx.save_for_backward(dl)
        ctx.shape = logits.shape
        return loss

    @staticmethod
    def backward(ctx, g):
        (dl,) = ctx.saved_tensors
        return (dl * g).view(ctx.shape), None, None


class ScaleAndShiftInvariantLoss(nn.Module):
    def __init__(self, alpha=0.5, scales=4, reduction="batch-based"):
        super().__init__()
        if reduction != "batch-based":
            raise NotImplementedError("the reference trains with the batch-based reduction only")
        self.alpha = alpha
        self.scales = scales
        self.prediction_ssi = None

    def forward(self, prediction, target):
        prediction = prediction.squeeze(1).float()
        target = target.squeeze(1).float()
        if _fused_ok(prediction, target) and 1 <= self.scales <= 4:
            self.prediction_ssi = None  # not materialised by the fused kernels
            return _SsiFn.apply(prediction, target, self.alpha, self.scales)
        mask = target > 0
        scale, shift = compute_scale_and_shift(prediction, target, mask)
        ssi = scale.view(-1, 1, 1) * prediction + shift.view(-1, 1, 1)
        self.prediction_ssi = ssi
        total = mse_loss(ssi, target, mask)
        if self.alpha > 0:
            reg = 0
            for s in range(self.scales):
                step = 2 ** s
                reg = reg + gradient_loss(ssi[:, ::step, ::step], target[:, ::step, ::step],
                                          mask[:, ::step, ::step])
            total = total + self.alpha * reg
        return total


class SoftDiceLoss(torch.nn.Module):
    """Mirror of `Binary_segmentation/Metrics/losses.py:5-24` (host-side loss reduction): soft Dice
    on sigmoid(logits), mean over the batch."""

    def __init__(self, smooth=1e-8):
        super().__init__()
        self.smooth = smooth

    def forward(self, logits, targets):
        if _fused_ok(logits, targets):
            return _DiceFn.apply(logits, targets, self.smooth)
        num = targets.size(0)
        m1 = torch.sigmoid(logits).view(num, -1)
        m2 = targets.view(num, -1)
        score = 2.0 * ((m1 * m2).sum(1) + self.smooth) / ((m1 * m1).sum(1) + (m2 * m2).sum(1) + self.smooth)
        return 1 - score.sum() / num


class _CeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, weight):
        from . import _lib
        from .ops import ptr, stream
        L = _lib.load()
        x = logits.contiguous().float()
        t = target.contiguous()
        w = None if weight is None else weight.to(device=x.device, dtype=torch.float32).contiguous()
        B, C = x.shape
        ws = torch.empty(L.ssl4gie_cross_entropy_workspace_bytes(B, C), dtype=torch.uint8, device=x.device)
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        dx = torch.empty_like(x)
        _lib.check(L.ssl4gie_cross_entropy(ptr(x), ptr(t), ptr(w), ptr(loss), ptr(dx), B, C, ptr(ws), stream()),
                   "cross_entropy")
        ctx.save_for_backward(dx)
        ctx.dtype = logits.dtype
        return loss

    @staticmethod
    def backward(ctx, g):
        (dx,) = ctx.saved_tensors
        return (dx * g).to(ctx.dtype), None, None


class CrossEntropyLoss(nn.Module):
    """`nn.CrossEntropyLoss(weight)` of the classification finetune (`train_classification.py:278`), mean
    reduction: one fused value-and-gradient kernel pair for fp32 / bf16 logits [B, C] with int64 class targets on
    the device; the torch formulation for CPU tensors, SSL4GIE_FUSED_LOSS=0 and every other input rank."""

    def __init__(self, weight=None):
        super().__init__()
        self.register_buffer("weight", None if weight is None else torch.as_tensor(weight, dtype=torch.float32))

    def forward(self, logits, target):
        if (_fused_ok(logits, target) and logits.dim() == 2 and target.dim() == 1
                and target.dtype == torch.int64 and logits.dtype in (torch.float32, torch.bfloat16)):
            return _CeFn.apply(logits, target, self.weight)
        w = self.weight
        if w is not None and w.dtype != logits.dtype:
            w = w.to(logits.dtype)
        return nn.functional.cross_entropy(logits, target, weight=w)


class _InfoNceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k_all, T, label_offset):
        from . import _lib
        from .ops import ptr, stream
        L = _lib.load()
        qf = q.contiguous().float()
        kf = k_all.detach().contiguous().float()
        (N, C), M = qf.shape, kf.shape[0]
        ws = torch.empty(L.ssl4gie_infonce_workspace_bytes(N, M, C), dtype=torch.uint8, device=qf.device)
        loss = torch.empty((), dtype=torch.float32, device=qf.device)
        dq = torch.empty_like(qf)
        _lib.check(L.ssl4gie_infonce_loss(ptr(qf), ptr(kf), ptr(loss), ptr(dq), N, M, C, float(T), int(label_offset),
                                          ptr(ws), stream()), "infonce_loss")
        ctx.save_for_backward(dq)
        ctx.dtype = q.dtype
        return loss

    @staticmethod
    def backward(ctx, g):
        (dq,) = ctx.saved_tensors
        return (dq * g).to(ctx.dtype), None, None, None


def info_nce_normalized(q, k_all, T, label_offset=0):
    """the tail of the reference's `MoCo.contrastive_loss` (builder.py:68-73) on rows that are already
    L2-normalised: logits = q k_all^T / T, labels = arange(n) + label_offset, cross entropy x 2T (torch ops)"""
    if q.is_cuda:
        from .engine import MatmulNTFn
        logits = MatmulNTFn.apply(q, k_all) / T  # einsum('nc,mc->nm') of builder.py:83
    else:
        logits = q @ k_all.t() / T
    n = logits.shape[0]  # batch size per GPU
    labels = torch.arange(n, dtype=torch.long, device=logits.device) + label_offset
    return nn.functional.cross_entropy(logits, labels) * (2 * T)


def info_nce(q, k_all, T, label_offset=0):
    """MoCo-v3's InfoNCE (`builder.py:63-73`): q [N, C] queries, k_all [M, C] the gathered keys of all ranks (no
    gradient), row i's positive key is `label_offset + i`.  On the device one fused kernel chain (row norms, online
    softmax over key chunks, dq through the normalisation; the [N, M] logits never reach memory); the torch
    formulation for CPU tensors, keys that require a gradient, C > 1024 or SSL4GIE_FUSED_LOSS=0."""
    if (_fused_ok(q, k_all) and q.dim() == 2 and k_all.dim() == 2 and not k_all.requires_grad
            and q.shape[1] == k_all.shape[1] and q.shape[1] <= 1024):
        return _InfoNceFn.apply(q, k_all, T, label_offset)
    return info_nce_normalized(nn.functional.normalize(q, dim=1), nn.functional.normalize(k_all, dim=1), T,
                               label_offset)


class _SoftCeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, soft_target, label, smoothing):
        from . import _lib
        from .ops import ptr, stream
        L = _lib.load()
        x = logits.contiguous().float()
        B, C = x.shape
        t = None if soft_target is None else soft_target.contiguous().float()
        lab = None if label is None else label.contiguous()
        conf, off = (1.0 - smoothing, smoothing / C) if label is not None else (0.0, 0.0)
        ws = torch.empty(L.ssl4gie_soft_cross_entropy_workspace_bytes(B, C), dtype=torch.uint8, device=x.device)
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        dx = torch.empty_like(x)
        _lib.check(L.ssl4gie_soft_cross_entropy(ptr(x), ptr(t), ptr(lab), conf, off, ptr(loss), ptr(dx), B, C, ptr(ws),
                                                stream()), "soft_cross_entropy")
        ctx.save_for_backward(dx)
        ctx.dtype = logits.dtype
        return loss

    @staticmethod
    def backward(ctx, g):
        (dx,) = ctx.saved_tensors
        return (dx * g).to(ctx.dtype), None, None, None


def _soft_ce_fused_ok(logits, other, other_dtype):
    return (_fused_ok(logits, other) and logits.dim() == 2 and other.dtype == other_dtype
            and logits.dtype in (torch.float32, torch.bfloat16))


class SoftTargetCrossEntropy(nn.Module):
    """timm's `SoftTargetCrossEntropy` (the criterion behind Mixup, `main_finetune.py:292`):
    mean_b sum_c -target[b, c] log_softmax(x[b])[c]; the targets get no gradient.  One fused value-and-gradient
    kernel pair for fp32 / bf16 logits [B, C] with fp32 targets [B, C] on the device; the torch formulation for CPU
    tensors, SSL4GIE_FUSED_LOSS=0 and every other rank or dtype."""

    def forward(self, x, target):
        if _soft_ce_fused_ok(x, target, torch.float32) and target.shape == x.shape and not target.requires_grad:
            return _SoftCeFn.apply(x, target, None, 0.0)
        return torch.sum(-target * nn.functional.log_softmax(x, dim=-1), dim=-1).mean()


class LabelSmoothingCrossEntropy(nn.Module):
    """timm's `LabelSmoothingCrossEntropy` (`main_finetune.py:294`): (1 - smoothing) nll + smoothing mean_c(-log p),
    mean over the batch — the soft-target kernel with the target row built from the int64 label inside it; the torch
    formulation elsewhere (see SoftTargetCrossEntropy)."""

    def __init__(self, smoothing=0.1):
        super().__init__()
        assert smoothing < 1.0
        self.smoothing = smoothing
        self.confidence = 1. - smoothing

    def forward(self, x, target):
        if _soft_ce_fused_ok(x, target, torch.int64) and target.dim() == 1 and target.shape[0] == x.shape[0]:
            return _SoftCeFn.apply(x, None, target, float(self.smoothing))
        logp = nn.functional.log_softmax(x, dim=-1)
        nll = -logp.gather(dim=-1, index=target.unsqueeze(1)).squeeze(1)
        return (self.confidence * nll + self.smoothing * -logp.mean(dim=-1)).mean()
