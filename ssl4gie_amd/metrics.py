"""Evaluation metrics of the three finetune heads: what the drivers' `test()` loops and the `eval_*.py` CLIs compute.

Same class / function names and call signatures as the reference's `Binary_segmentation/Metrics/performance.py`
(DiceScore, IoU, Precision, Recall), `Classification/Metrics/performance.py` (meanF1Score, meanPrecision, meanRecall)
and `Depth_estimation/eval_depth.py:19-28` (rmse, rel_err, abs_err) — except that every result is a 0-dim tensor on the
input's device and the caller decides when to read it back (`.item()`).

On the HIP device the work runs in the kernels of csrc/metric_ops.hip: one pass counts |m1|, |m2|, |m1 & m2| for all
four segmentation scores (resampling the logits to the target's size on the fly), the classification means come from a
confusion matrix that adds up over a loader, and the depth errors come from one fused pass per image with the median
by an exact radix select.  The accumulators `SegmentationScores`, `ClassificationScores` and `DepthErrors` keep their
state on the device and synchronise only in `.compute()`.  CPU tensors, or SSL4GIE_FUSED_METRICS=0, take the torch
formulation below, which restates the reference line by line and is the parity reference of the kernels.

Two deliberate differences on the device path: `sigmoid(x) > 0.5` is decided as `x > 0` (the
reference's fp32 sigmoid is false for 0 < x <~ 1.2e-7 as well), and the bilinear resize is
F.interpolate(align_corners=False) without antialiasing — what TF.resize of a tensor does in the reference's pinned
torchvision 0.10, not what current torchvision does when it shrinks a map.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from .losses import compute_scale_and_shift


def _fused_ok(*ts):
    return all(t.is_cuda for t in ts) and os.environ.get("SSL4GIE_FUSED_METRICS", "1") != "0"


# ------------------------------------------------------------------ segmentation
def _seg_terms_torch(logits, targets, sigmoid):
    """performance.py:11-19 (the same lines in all four classes)"""
    num = targets.size(0)
    if sigmoid:
        probs = torch.sigmoid(logits)
    else:
        probs = logits
    m1 = probs.reshape(num, -1) > 0.5
    m2 = targets.reshape(num, -1) > 0.5
    intersection = m1 * m2
    return num, m1, m2, intersection


def _seg_scores_torch(logits, targets, sigmoid, smooth):
    """the four closing formulas (performance.py:21-26, :46-49, :69-70, :90-91), as a [4] tensor"""
    num, m1, m2, intersection = _seg_terms_torch(logits, targets, sigmoid)
    dice = 2.0 * (intersection.sum(1) + smooth) / (m1.sum(1) + m2.sum(1) + smooth)
    iou = (intersection.sum(1) + smooth) / (m1.sum(1) + m2.sum(1) - intersection.sum(1) + smooth)
    prec = (intersection.sum(1) + smooth) / (m1.sum(1) + smooth)
    rec = (intersection.sum(1) + smooth) / (m2.sum(1) + smooth)
    return torch.stack([s.sum() / num for s in (dice, iou, prec, rec)]), torch.stack([dice, iou, prec, rec])


def _seg_operands(logits, targets):
    """[B, Hin, Win] logits (fp32 / bf16) and [B, H, W] targets (fp32 / uint8) for ops.seg_counts"""
    num = targets.size(0)

    def maps(t):
        if t.dim() == 4 and t.shape[1] == 1:
            return t.reshape(num, t.shape[2], t.shape[3])
        if t.dim() == 3:
            return t
        return t.reshape(num, 1, -1)
    l, t = maps(logits), maps(targets)
    if l.dtype not in (torch.float32, torch.bfloat16):
        l = l.float()
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    elif t.dtype not in (torch.float32, torch.uint8):
        t = t.float()
    return l.contiguous(), t.contiguous()


def _seg_scores_fused(logits, targets, sigmoid, smooth, accum=None):
    from . import ops
    l, t = _seg_operands(logits, targets)
    if l.shape[1:] != t.shape[1:] and l.numel() == t.numel():  # same pixels under another view: the reference's .view
        l = l.reshape(t.shape)
    return ops.seg_scores(ops.seg_counts(l, t, sigmoid), smooth, accum)


class _SegScore(nn.Module):
    _index = 0

    def __init__(self, smooth=1e-8):
        super().__init__()
        self.smooth = smooth

    def forward(self, logits, targets, sigmoid=True):
        if _fused_ok(logits, targets):
            return _seg_scores_fused(logits, targets, sigmoid, self.smooth)[self._index]
        return _seg_scores_torch(logits, targets, sigmoid, self.smooth)[0][self._index]


class DiceScore(_SegScore):
    """`performance.py:5-27`; an empty prediction on an empty target scores 2.0, as there"""
    _index = 0


class IoU(_SegScore):
    """`performance.py:30-50`"""
    _index = 1


class Precision(_SegScore):
    """`performance.py:53-71`"""
    _index = 2


class Recall(_SegScore):
    """`performance.py:74-92`"""
    _index = 3


class SegmentationScores:
    """Dice, IoU, precision and recall over a whole loader (eval_segmentation.py:27-43, and the `test()` of
    train_segmentation.py): `update` resamples the logits to the target's stored size where they differ (the
    reference's TF.resize at :36-37), scores the batch and adds the per-image scores to a device accumulator — two
    launches, no read-back; it returns the batch's four mean scores as a device tensor.  `compute()` reads the means
    over all images back, the one synchronisation."""
    names = ("dice", "iou", "precision", "recall")

    def __init__(self, smooth=1e-8):
        self.smooth = smooth
        self.accum = None

    def reset(self):
        self.accum = None

    def update(self, logits, target, size=None):
        hw = tuple(target.shape[-2:])
        if size is not None and tuple(size) != hw:
            raise ValueError(f"size {tuple(size)} is not the target's {hw}")
        if self.accum is None:
            self.accum = torch.zeros(5, dtype=torch.float64, device=logits.device)
        if _fused_ok(logits, target):
            return _seg_scores_fused(logits, target, True, self.smooth, self.accum)
        if logits.dim() == 4 and tuple(logits.shape[-2:]) != hw:
            logits = F.interpolate(logits.float(), size=hw, mode="bilinear", align_corners=False)
        mean, per_image = _seg_scores_torch(logits, target, True, self.smooth)
        self.accum[:4] += per_image.double().sum(1)
        self.accum[4] += target.size(0)
        return mean

    def compute(self):
        if self.accum is None:
            return {k: float("nan") for k in self.names}
        a = self.accum.cpu()
        return {k: float(a[i] / a[4]) for i, k in enumerate(self.names)}


# ------------------------------------------------------------------ classification
def _class_scores_torch(preds, targets, n_class, smooth):
    """the three per-class loops of Classification/Metrics/performance.py:10-22, :31-39, :48-56, side by side"""
    f1 = prec = rec = 0
    for i in range(n_class):
        m1 = preds == i
        m2 = targets == i
        intersection = m1 * m2
        f1 += 2.0 * (intersection.sum() + smooth) / (m1.sum() + m2.sum() + smooth)
        prec += (intersection.sum() + smooth) / (m1.sum() + smooth)
        rec += (intersection.sum() + smooth) / (m2.sum() + smooth)
    return f1 / n_class, prec / n_class, rec / n_class


def _confusion_fused(x, targets, n_class, conf=None):
    from . import ops
    if conf is None:
        conf = torch.zeros(n_class * n_class + 1, dtype=torch.int64, device=x.device)
    if x.dtype not in (torch.int64, torch.float32, torch.bfloat16):
        x = x.long() if not x.is_floating_point() else x.float()
    return ops.confusion_update(conf, x.contiguous(), targets.long().contiguous())


class _ClassScore(nn.Module):
    _index = 0

    def __init__(self, n_class, smooth=1e-8):
        super().__init__()
        self.n_class = n_class
        self.smooth = smooth

    def forward(self, preds, targets):
        if _fused_ok(preds, targets) and preds.dim() == 1:
            from . import ops
            return ops.confusion_scores(_confusion_fused(preds, targets, self.n_class), self.smooth)[self._index]
        return _class_scores_torch(preds, targets, self.n_class, self.smooth)[self._index]


class meanF1Score(_ClassScore):
    """`Classification/Metrics/performance.py:4-22`; a class absent from predictions and targets adds 2.0"""
    _index = 0


class meanPrecision(_ClassScore):
    """`Classification/Metrics/performance.py:25-39`"""
    _index = 1


class meanRecall(_ClassScore):
    """`Classification/Metrics/performance.py:42-56`"""
    _index = 2


class ClassificationScores:
    """Mean F1 / precision / recall and accuracy over a whole loader from one confusion matrix on the device, instead
    of the concatenate-and-rescore loop of train_classification.py:88-98 (quadratic in the number of batches, one
    `.item()` per batch).  `update` takes logits [B, C] (argmax = first maximum) or predictions int64 [B]; a target or
    prediction outside [0, C) is counted as rejected and leaves the matrix alone."""
    names = ("f1", "precision", "recall", "accuracy")

    def __init__(self, n_class, smooth=1e-8):
        self.n_class = n_class
        self.smooth = smooth
        self.conf = None

    def reset(self):
        self.conf = None

    def update(self, logits_or_preds, targets):
        x, C = logits_or_preds, self.n_class
        if self.conf is None:
            self.conf = torch.zeros(C * C + 1, dtype=torch.int64, device=x.device)
        if _fused_ok(x, targets):
            _confusion_fused(x, targets, C, self.conf)
            return
        preds = torch.argmax(x, 1) if x.dim() == 2 else x
        ok = (targets >= 0) & (targets < C) & (preds >= 0) & (preds < C)
        flat = torch.where(ok, targets * C + preds, torch.full_like(targets, C * C))
        self.conf += torch.bincount(flat, minlength=C * C + 1)

    @property
    def matrix(self):
        C = self.n_class
        return None if self.conf is None else self.conf[:C * C].view(C, C)

    def scores(self):
        """fp32 [4] on the accumulator's device: mean F1, mean precision, mean recall, accuracy; no synchronisation"""
        if self.conf is None:
            raise RuntimeError("ClassificationScores.scores() before the first update")
        if _fused_ok(self.conf):
            from . import ops
            return ops.confusion_scores(self.conf, self.smooth)
        m, s = self.matrix, self.smooth
        tp, m1, m2 = m.diagonal(), m.sum(0), m.sum(1)
        f1 = prec = rec = 0
        for i in range(self.n_class):  # the reference's terms and summation order
            f1 += 2.0 * (tp[i] + s) / (m1[i] + m2[i] + s)
            prec += (tp[i] + s) / (m1[i] + s)
            rec += (tp[i] + s) / (m2[i] + s)
        n = self.n_class
        return torch.stack([f1 / n, prec / n, rec / n, tp.sum() / m.sum()]).float()

    def compute(self):
        if self.conf is None:
            return {**{k: float("nan") for k in self.names}, "rejected": 0}
        s = self.scores().cpu()
        return {**{k: float(s[i]) for i, k in enumerate(self.names)}, "rejected": int(self.conf[-1])}


# ------------------------------------------------------------------ depth
def lower_median(x):
    """torch.median's lower median (the element of rank (n - 1) // 2) of non-negative values as a 0-dim tensor; NaN for
    an empty x.  On the device an exact radix select instead of a sort; x is not modified."""
    if _fused_ok(x):
        from . import ops
        return ops.lower_median(x.reshape(-1).float().contiguous())
    if x.numel() == 0:
        return torch.full((), float("nan"), dtype=torch.float32, device=x.device)
    return torch.median(x)


def rmse(pred, targ):
    """`eval_depth.py:19-20` without the `.item()`"""
    return torch.sqrt(torch.mean((pred - targ)[targ > 0] ** 2))


def rel_err(pred, targ):
    """`eval_depth.py:23-24` without the `.item()`; the median is `lower_median` (a select on the device)"""
    return lower_median(torch.abs((pred - targ) / targ)[targ > 0])


def abs_err(pred, targ):
    """`eval_depth.py:27-28` without the `.item()`"""
    return torch.mean(torch.abs(pred - targ)[targ > 0])


def crop_offset(big, small):
    """torchvision's centre-crop offset (`int(round((big - small) / 2.0))`: Python rounds a half to even)"""
    return int(round((big - small) / 2.0))


def _maps3(t):
    return t.reshape(t.shape[0], t.shape[-2], t.shape[-1])


def depth_errors_torch(pred, target, target_og, scale_):
    """eval_depth.py:43-61 line by line for a batch, the three errors per image as fp32 [B, 3].  The resize is
    F.interpolate(bilinear, align_corners=False) and the centre crop a slice at torchvision's offsets; target_og is not
    modified (the reference scales it in place)."""
    output, target, target_og = _maps3(pred).float(), _maps3(target).float(), _maps3(target_og).float()
    scale, shift = compute_scale_and_shift(output, target, target > 0.0)
    output = scale.view(-1, 1, 1) * output + shift.view(-1, 1, 1)
    h, w = target_og.shape[1], target_og.shape[2]
    max_size = max(h, w)
    output = F.interpolate(output.unsqueeze(1), size=(max_size, max_size), mode="bilinear", align_corners=False)
    top, left = crop_offset(max_size, h), crop_offset(max_size, w)
    output = output[:, 0, top:top + h, left:left + w].clone()
    output[output < 0.0] = 0.0
    output[output > 1.0] = 1.0
    output[target_og == 0.0] = 0.0
    output = output * scale_
    target_og = target_og * scale_
    rows = [torch.stack([rmse(o, t), rel_err(o, t), abs_err(o, t)]) for o, t in zip(output, target_og)]
    return torch.stack(rows)


class DepthErrors:
    """RMSE, median relative error and mean absolute error over a whole loader (eval_depth.py:31-61).  `update` takes
    the model's prediction and the training-size target [B, 1, S, S] (or [B, S, S]) and the stored-size target
    [B, 1, H, W]; on the device the alignment, resize, crop, clamp, mask, the three reductions and the median run in
    one kernel chain without a read-back.  Returns the batch's errors fp32 [B, 3]; `compute()` reads the means over
    all images back."""
    names = ("rmse", "rel_err", "abs_err")

    def __init__(self, scale=10.0):
        self.scale = scale
        self.accum = None

    def reset(self):
        self.accum = None

    def update(self, pred, target, target_og):
        if _fused_ok(pred, target, target_og):
            from . import ops
            out = ops.depth_eval(_maps3(pred).float().contiguous(), _maps3(target).float().contiguous(),
                                 _maps3(target_og).float().contiguous(), self.scale)
        else:
            out = depth_errors_torch(pred, target, target_og, self.scale)
        if self.accum is None:
            self.accum = torch.zeros(4, dtype=torch.float64, device=out.device)
        self.accum[:3] += out.double().sum(0)
        self.accum[3] += out.shape[0]
        return out

    def compute(self):
        if self.accum is None:
            return {k: float("nan") for k in self.names}
        a = self.accum.cpu()
        return {k: float(a[i] / a[3]) for i, k in enumerate(self.names)}
