"""Evaluation metrics of the four finetune tasks: what the drivers' `test()` loops and the `eval_*.py` CLIs compute.

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

The linear-probe drivers score with `accuracy(output, target, topk=(1, 5))` and one `.item()` per meter per batch
(`Models/moco_v3/main_lincls.py:365-373,506-520`, `Models/mae/engine_finetune.py:119-124`): `accuracy` here has that
signature and returns device tensors, and `TopKAccuracy` adds hits per k, rows and the cross-entropy sum up on the
device over a loader (csrc/probe_ops.hip) with one read-back.  Equal logits are ordered by lower index first — the rule
of the argmax above — where `torch.topk` leaves ties open.

The detection drivers (`Object_detection/train_detection.py:113-151`, `eval_detection.py:21-44`) score with torchmetrics'
`MeanAveragePrecision()`; the class of that name here takes the same `update(preds, target)` / `compute()` calls, keeps
the detections of a loader on the device and runs COCO's evaluation in the kernels of csrc/det_map_ops.hip.

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

from . import _lib
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


# ------------------------------------------------------------------ top-k accuracy (the linear-probe drivers)
def _check_topk(topk, C):
    ks = [int(k) for k in topk]
    if not 1 <= len(set(ks)) <= 8 or min(ks) < 1:
        raise ValueError(f"topk must hold 1 to 8 distinct values >= 1, got {tuple(topk)}")
    if max(ks) > C:
        raise ValueError(f"topk={tuple(topk)} asks for more than the C = {C} classes of the logits")
    return ks


def topk_ranks_torch(logits, target):
    """the rank rule of ssl4gie_topk_update in torch ops: (rank int64 [B], ok bool [B], loss fp32 [B]).  rank = the
    number of columns ordered above the target's logit — equal values by lower index first, a NaN above every number,
    NaNs among themselves by lower index first (`torch.topk` leaves the order of ties open); ok = target in [0, C);
    loss = the row's cross-entropy in fp32.  Rows that are not ok hold rank -1 and loss 0."""
    x = logits.float()
    B, C = x.shape
    ok = (target >= 0) & (target < C)
    t = target.clamp(0, C - 1).view(B, 1)
    xt = x.gather(1, t)
    xnan, tnan = x.isnan(), xt.isnan()
    over = ~tnan & (xnan | (x > xt))
    tie = torch.where(tnan, xnan, x == xt)
    col = torch.arange(C, device=x.device).view(1, C)
    rank = (over | (tie & (col < t))).sum(1)
    loss = F.cross_entropy(x, t.view(B), reduction="none")
    return torch.where(ok, rank, torch.full_like(rank, -1)), ok, torch.where(ok, loss, torch.zeros_like(loss))


def _topk_state(nk, device):
    """int64 [nk + 3] in ONE buffer: hits per k, rows counted, rows rejected, and the fp64 loss sum's bits"""
    state = torch.zeros(nk + 3, dtype=torch.int64, device=device)
    return state, state[:nk + 2], state[nk + 2:].view(torch.float64)


def _topk_update(acc, loss_sum, logits, target, ks, workspace=None):
    if logits.dim() != 2 or target.dim() != 1 or logits.shape[0] != target.shape[0]:
        raise ValueError(f"logits [B, C] and target [B] expected, got {tuple(logits.shape)}, {tuple(target.shape)}")
    if _fused_ok(logits, target) and logits.shape[0]:
        from . import ops
        if logits.dtype not in (torch.float32, torch.bfloat16):
            logits = logits.float()
        ops.topk_update(acc, loss_sum, logits, target.long().contiguous(), ks, workspace=workspace)
        return
    rank, ok, loss = topk_ranks_torch(logits, target.long())
    hits = [(ok & (rank < k)).sum() for k in ks]
    acc += torch.stack(hits + [ok.sum(), (~ok).sum()])
    loss_sum += loss.double().sum()


@torch.no_grad()
def accuracy(output, target, topk=(1,)):
    """the drivers' `accuracy(output, target, topk=(1, 5))` (Models/moco_v3/main_lincls.py:506-520; timm's, imported at
    Models/mae/engine_finetune.py:19): the precision@k of one batch in percent, a list of fp32 [1] tensors on the
    logits' device — nothing is read back.  Ties are ordered by lower index first where `topk` leaves them open."""
    ks = _check_topk(topk, output.shape[1])
    order = sorted(set(ks))
    _, acc, loss_sum = _topk_state(len(order), output.device)
    _topk_update(acc, loss_sum, output, target, order)
    scale = 100.0 / max(1, target.shape[0])
    return [acc[order.index(k):order.index(k) + 1].float() * scale for k in ks]


class TopKAccuracy:
    """acc@k and the mean cross-entropy over a whole loader from device accumulators, instead of the drivers'
    `accuracy(...)` + one `.item()` per meter per batch (main_lincls.py:365-368, engine_finetune.py:119-124).
    `update(logits [B, C], target [B])` adds a batch (fp32 or bf16 logits, any row stride); `compute()` is the ONE
    read-back: {"acc1": .., "acc5": .., "loss": .., "n": .., "rejected": ..}, accuracies in percent of the n rows
    counted; a target outside [0, C) is counted as rejected and adds to nothing else."""

    def __init__(self, topk=(1, 5)):
        ks = [int(k) for k in topk]
        if not 1 <= len(ks) <= 8 or ks[0] < 1 or any(b <= a for a, b in zip(ks, ks[1:])):
            raise ValueError(f"topk must hold 1 to 8 strictly ascending values >= 1, got {tuple(topk)}")
        self.topk = tuple(ks)
        self.state = self._acc = self._loss = self._ws = None

    def reset(self):
        self.state = self._acc = self._loss = None

    def update(self, logits, target):
        _check_topk(self.topk, logits.shape[1])
        if self.state is None:
            self.state, self._acc, self._loss = _topk_state(len(self.topk), logits.device)
        if _fused_ok(logits, target):  # the row-loss workspace is kept across batches
            need = _lib.load().ssl4gie_topk_workspace_bytes(logits.shape[0])
            if self._ws is None or self._ws.device != logits.device or self._ws.numel() < need:
                from . import ops
                self._ws = ops.topk_workspace(logits.shape[0], logits.device)
        _topk_update(self._acc, self._loss, logits, target, list(self.topk), self._ws)

    def compute(self):
        names = [f"acc{k}" for k in self.topk]
        if self.state is None:
            return {**{k: float("nan") for k in names}, "loss": float("nan"), "n": 0, "rejected": 0}
        host = self.state.cpu()
        nk = len(self.topk)
        n, rejected = int(host[nk]), int(host[nk + 1])
        loss_sum = float(host[nk + 2:].view(torch.float64)[0])
        out = {k: (100.0 * int(host[i]) / n if n else float("nan")) for i, k in enumerate(names)}
        return {**out, "loss": loss_sum / n if n else float("nan"), "n": n, "rejected": rejected}


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


# ------------------------------------------------------------------ detection: COCO mean average precision
_MAP_NAMES = ("map", "map_50", "map_75", "map_small", "map_medium", "map_large", "mar_1", "mar_10", "mar_100",
              "mar_small", "mar_medium", "mar_large")
_MAP_AREAS = ((0.0, 1e10), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10))   # all, small, medium, large
_MAP_MAX_DETS = (1, 10, 100)
MAP_MAX_PER_IMAGE = _lib.DET_MAP_MAX_PER_IMAGE    # detections, and ground truths, of one image
MAP_MAX_LABEL = _lib.DET_MAP_CLASSES - 1


def _map_xywh(boxes):
    """box_convert(xyxy -> xywh) on the fp32 tensor, then fp64"""
    wh = boxes[:, 2:] - boxes[:, :2]
    return torch.cat([boxes[:, :2], wh], 1).double()


def _map_iou(d, g):
    """pycocotools' bbIou on xywh boxes, fp64 [D, G]"""
    w = torch.minimum((d[:, 0] + d[:, 2])[:, None], (g[:, 0] + g[:, 2])[None]) - torch.maximum(d[:, None, 0], g[None, :, 0])
    h = torch.minimum((d[:, 1] + d[:, 3])[:, None], (g[:, 1] + g[:, 3])[None]) - torch.maximum(d[:, None, 1], g[None, :, 1])
    inter = w * h
    union = (d[:, 2] * d[:, 3])[:, None] + (g[:, 2] * g[:, 3])[None] - inter
    return torch.where((w > 0) & (h > 0), inter / union, torch.zeros_like(inter))


def _map_match_torch(d, g, thr, lo, hi):
    """COCOeval.evaluateImg for one image and class, the 4 areas x 10 thresholds side by side: d fp64 [D, 4] best
    first, g fp64 [G, 4].  Returns dtm, dt_ig bool [4, 10, D] and the ground truths' ignore flags [4, G]."""
    D, G = d.shape[0], g.shape[0]
    d_out = ((d[:, 2] * d[:, 3])[None] < lo[:, None]) | ((d[:, 2] * d[:, 3])[None] > hi[:, None])       # [4, D]
    g_ig = ((g[:, 2] * g[:, 3])[None] < lo[:, None]) | ((g[:, 2] * g[:, 3])[None] > hi[:, None])        # [4, G]
    dtm = torch.zeros(4, thr.numel(), D, dtype=torch.bool, device=d.device)
    dt_ig = d_out[:, None, :].expand(4, thr.numel(), D).clone()
    if D == 0 or G == 0:
        return dtm, dt_ig, g_ig
    ious = _map_iou(d, g)
    gtm = torch.zeros(4, thr.numel(), G, dtype=torch.bool, device=d.device)
    first = torch.clamp(thr, max=1 - 1e-10)[None, :, None]
    ar = torch.arange(G, device=d.device)

    def last_best(cand, row):
        # walking the candidates in order and taking every IoU >= the best so far ends on the last of the largest
        val = torch.where(cand, row, torch.full_like(row, -1.0))
        best = val.max(-1, keepdim=True).values
        idx = torch.where(cand & (val == best), ar, torch.full_like(ar, -1)).max(-1).values
        return idx, idx >= 0

    for k in range(D):
        row = ious[k].expand(4, thr.numel(), G)
        cand = (row >= first) & ~gtm
        # the ground truths are sorted non-ignored first, and the walk stops where the ignored ones begin once it
        # holds a regular match
        m_reg, has_reg = last_best(cand & ~g_ig[:, None, :], row)
        m_ign, has_ign = last_best(cand & g_ig[:, None, :], row)
        m = torch.where(has_reg, m_reg, m_ign)
        has = has_reg | has_ign
        dtm[:, :, k] = has
        dt_ig[:, :, k] = torch.where(has, ~has_reg, dt_ig[:, :, k])
        gtm |= has[..., None] & (ar == m[..., None])
    return dtm, dt_ig, g_ig


def _map_torch(det_boxes, det_scores, det_labels, n_det, gt_boxes, gt_labels, n_gt, iou_thr, rec_thr):
    """The rule of MeanAveragePrecision's docstring in torch ops, in pycocotools' order of steps: fp64 [12] on the
    inputs' device, and the classes as a list."""
    dev = det_boxes.device
    thr = torch.tensor(iou_thr, dtype=torch.float64, device=dev)
    rec = torch.tensor(rec_thr, dtype=torch.float64, device=dev)
    lo = torch.tensor([a[0] for a in _MAP_AREAS], dtype=torch.float64, device=dev)
    hi = torch.tensor([a[1] for a in _MAP_AREAS], dtype=torch.float64, device=dev)
    classes = torch.unique(torch.cat([det_labels, gt_labels])).tolist()
    T, R, K = thr.numel(), rec.numel(), len(classes)
    precision = -torch.ones(T, R, K, 4, 3, dtype=torch.float64, device=dev)
    recall = -torch.ones(T, K, 4, 3, dtype=torch.float64, device=dev)
    d_xywh, g_xywh = _map_xywh(det_boxes), _map_xywh(gt_boxes)
    d_start = [0]
    for n in n_det:
        d_start.append(d_start[-1] + n)
    g_start = [0]
    for n in n_gt:
        g_start.append(g_start[-1] + n)
    # which detections and ground truths of which image carry which class: planned once on the host
    det_labels_h, gt_labels_h = det_labels.cpu().numpy(), gt_labels.cpu().numpy()
    groups = {c: [] for c in classes}
    for i in range(len(n_det)):
        dl, gl = det_labels_h[d_start[i]:d_start[i + 1]], gt_labels_h[g_start[i]:g_start[i + 1]]
        for c in sorted(set(dl.tolist()) | set(gl.tolist())):
            groups[c].append(((dl == c).nonzero()[0] + d_start[i], (gl == c).nonzero()[0] + g_start[i]))
    for k, c in enumerate(classes):
        scores, ranks, dtms, dtigs = [], [], [], []
        npig = torch.zeros(4, dtype=torch.int64, device=dev)
        for dsel, gsel in groups[c]:
            dsel, gsel = torch.from_numpy(dsel).to(dev), torch.from_numpy(gsel).to(dev)
            order = torch.sort(det_scores[dsel], descending=True, stable=True).indices[:_MAP_MAX_DETS[-1]]
            dsel = dsel[order]
            dtm, dt_ig, g_ig = _map_match_torch(d_xywh[dsel], g_xywh[gsel], thr, lo, hi)
            npig += (~g_ig).sum(1)
            scores.append(det_scores[dsel])
            ranks.append(torch.arange(dsel.numel(), device=dev))
            dtms.append(dtm)
            dtigs.append(dt_ig)
        scores, ranks = torch.cat(scores), torch.cat(ranks)
        dtm, dt_ig = torch.cat(dtms, 2), torch.cat(dtigs, 2)
        for m, max_det in enumerate(_MAP_MAX_DETS):
            keep = (ranks < max_det).nonzero().squeeze(1)
            inds = keep[torch.sort(scores[keep], descending=True, stable=True).indices]
            nd = inds.numel()
            for a in range(4):
                # (a class and area without a regular ground truth stays -1: the mask below)
                tps = (dtm[a][:, inds] & ~dt_ig[a][:, inds]).double().cumsum(1)
                fps = (~dtm[a][:, inds] & ~dt_ig[a][:, inds]).double().cumsum(1)
                n = npig[a].double()
                if nd:
                    rc = tps / n
                    pr = tps / (fps + tps + 2.220446049250313e-16)     # np.spacing(1)
                    pr = torch.cummax(pr.flip(1), 1).values.flip(1)
                    pos = torch.searchsorted(rc.contiguous(), rec[None].expand(T, R).contiguous(), side="left")
                    q = torch.where(pos < nd, torch.gather(pr, 1, pos.clamp(max=nd - 1)), torch.zeros_like(rec)[None])
                    r_last = rc[:, -1]
                else:
                    q = torch.zeros(T, R, dtype=torch.float64, device=dev)
                    r_last = torch.zeros(T, dtype=torch.float64, device=dev)
                some = npig[a] > 0
                precision[:, :, k, a, m] = torch.where(some, q, torch.full_like(q, -1.0))
                recall[:, k, a, m] = torch.where(some, r_last, torch.full_like(r_last, -1.0))

    def mean(s):
        ok = s > -1
        n = ok.sum()
        return torch.where(n > 0, (s * ok).sum() / n.clamp(min=1), torch.full((), -1.0, dtype=torch.float64, device=dev))

    out = [mean(precision[:, :, :, 0, 2]), mean(precision[0, :, :, 0, 2]), mean(precision[5, :, :, 0, 2]),
           mean(precision[:, :, :, 1, 2]), mean(precision[:, :, :, 2, 2]), mean(precision[:, :, :, 3, 2]),
           mean(recall[:, :, 0, 0]), mean(recall[:, :, 0, 1]), mean(recall[:, :, 0, 2]),
           mean(recall[:, :, 1, 2]), mean(recall[:, :, 2, 2]), mean(recall[:, :, 3, 2])]
    return torch.stack(out), classes


class MeanAveragePrecision:
    """COCO mean average precision and recall of a detector over a whole loader: `update(preds, target)` and
    `compute()` as the reference's loops call torchmetrics' class of this name (train_detection.py:113-151,
    eval_detection.py:21-44), with its defaults — the only configuration built; any other constructor value, and a
    target with `iscrowd` or `area`, raises NotImplementedError (`sync_on_compute` and torchmetrics' other cross-rank
    options are accepted and have nothing to act on: there is no cross-rank sync).

    `update` appends the batch to device buffers and per-image counts taken from `.shape`: it never synchronises.
    `preds`: a list of dicts with `boxes` fp32 [n, 4] (xyxy), `scores` fp32 [n], `labels` int64 [n]; `target`: a list of
    dicts with `boxes` and `labels`.  At most 1024 detections and 1024 ground truths per image, labels in [0, 255] (checked
    on the device: `compute()` raises ValueError from the flag that comes back with the classes — its one read-back).
    `compute()` returns torchmetrics 1.1.2's dict: twelve 0-dim fp32 tensors on the inputs' device, `map_per_class` and
    `mar_100_per_class` = -1, `classes` int32; `compute_f64()` the twelve as fp64, before the cast.

    The rule (pycocotools' COCOeval; torchmetrics and pycocotools are not in this project's image, so this boundary is
    unpinned but for the example of torchmetrics' docstring: DESIGN.md sections 4 and 8).  For every class c seen in a
    prediction or a target and every area range a in all [0, 1e10], small [0, 32^2], medium [32^2, 96^2], large
    [96^2, 1e10]:

    Per image with a detection or a ground truth of c: the detections of c are stably sorted by descending score and
    the first 100 kept; the ground truths of c get ignore = area < lo or area > hi and are stably sorted non-ignored
    first.  Width and height are the fp32 differences x2 - x1, y2 - y1; everything after that is fp64: area = w h,
    overlap width = min(x1 + w, x1' + w') - max(x1, x1') (height alike), IoU = 0 when either overlap side is <= 0, else
    inter / (area + area' - inter).  For each IoU threshold t of torch.linspace(0.5, 0.95, 10).tolist() each detection
    takes greedily, in order: best = min(t, 1 - 1e-10); walk the ground truths in their sorted order; skip those already
    matched at this t; stop once a non-ignored match is held and the ignored ones begin; skip iou < best, otherwise take
    it and raise best.  A matched detection inherits the ground truth's ignore flag; an unmatched one whose own area is
    outside the range is ignored.

    Per class, area and maxDet in (1, 10, 100): the first maxDet detections of every image, in `update` order, stably
    sorted by descending score; tp and fp are cumulative counts over the non-ignored detections, npig the number of
    non-ignored ground truths; rc = tp / npig, pr = tp / (tp + fp + np.spacing(1)), pr made non-increasing from the
    right; precision[t, r] = pr at the first index with rc >= recThr[r] (torch.linspace(0, 1, 101).tolist()), 0 without
    one; recall[t] = the last rc, 0 without detections; -1 throughout where npig == 0.

    Summaries: the mean over the entries > -1, or -1 without any.  map, map_50 (t index 0), map_75 (t index 5) and
    map_small / medium / large use maxDet 100; mar_1 / 10 / 100 the area `all`; mar_small / medium / large maxDet 100.

    CPU tensors, or SSL4GIE_FUSED_METRICS=0, take the torch formulation above (`_map_torch`)."""

    def __init__(self, box_format="xyxy", iou_type="bbox", iou_thresholds=None, rec_thresholds=None,
                 max_detection_thresholds=None, class_metrics=False, **metric_kwargs):
        # train_detection.py:330 passes sync_on_compute=False; torchmetrics' cross-rank options have nothing to act
        # on here (no cross-rank sync: the reference evaluates on rank 0 only) and are accepted as they are
        unknown = set(metric_kwargs) - {"sync_on_compute", "dist_sync_on_step", "process_group", "dist_sync_fn",
                                        "compute_on_cpu", "compute_with_cache", "distributed_available_fn"}
        if unknown:
            raise TypeError(f"MeanAveragePrecision: unexpected keyword arguments {sorted(unknown)}")
        if box_format != "xyxy" or iou_type != "bbox" or iou_thresholds is not None or rec_thresholds is not None or \
                max_detection_thresholds is not None or class_metrics:
            raise NotImplementedError("MeanAveragePrecision is built for torchmetrics' defaults only: box_format='xyxy', "
                                      "iou_type='bbox', default thresholds, class_metrics=False")
        self.iou_thresholds = torch.linspace(0.5, 0.95, 10).tolist()
        self.rec_thresholds = torch.linspace(0.0, 1.0, 101).tolist()
        self.reset()

    def reset(self):
        self._det = ([], [], [])   # boxes, scores, labels: one tensor per update
        self._gt = ([], [])
        self._n_det, self._n_gt = [], []
        self._device = None

    @staticmethod
    def _check(t, dtype, shape_tail, what):
        if not torch.is_tensor(t) or t.dtype != dtype:
            raise ValueError(f"{what} must be a {dtype} tensor, got {getattr(t, 'dtype', type(t))}")
        if t.dim() != 1 + len(shape_tail) or tuple(t.shape[1:]) != shape_tail:
            raise ValueError(f"{what} must have shape [n{''.join(', %d' % s for s in shape_tail)}], got {tuple(t.shape)}")

    def update(self, preds, target):
        if not isinstance(preds, (list, tuple)) or not isinstance(target, (list, tuple)):
            raise ValueError("preds and target must be lists of dicts")
        if len(preds) != len(target):
            raise ValueError(f"preds holds {len(preds)} images, target {len(target)}")
        if not preds:
            return
        for p, t in zip(preds, target):
            if any(k not in p for k in ("boxes", "scores", "labels")) or any(k not in t for k in ("boxes", "labels")):
                raise ValueError("a prediction needs boxes, scores and labels, a target boxes and labels")
            if "iscrowd" in t or "area" in t:
                raise NotImplementedError("targets with iscrowd or area are not built")
            self._check(p["boxes"], torch.float32, (4,), "prediction boxes")
            self._check(p["scores"], torch.float32, (), "scores")
            self._check(p["labels"], torch.int64, (), "prediction labels")
            self._check(t["boxes"], torch.float32, (4,), "target boxes")
            self._check(t["labels"], torch.int64, (), "target labels")
            n, g = p["boxes"].shape[0], t["boxes"].shape[0]
            if p["scores"].shape[0] != n or p["labels"].shape[0] != n or t["labels"].shape[0] != g:
                raise ValueError("boxes, scores and labels of one image differ in length")
            if n > MAP_MAX_PER_IMAGE or g > MAP_MAX_PER_IMAGE:
                raise ValueError(f"at most {MAP_MAX_PER_IMAGE} detections and ground truths per image, got {n} and {g}")
            dev = self._device if self._device is not None else p["boxes"].device
            if any(x.device != dev for x in (p["boxes"], p["scores"], p["labels"], t["boxes"], t["labels"])):
                raise ValueError("all tensors of a MeanAveragePrecision must lie on one device")
            self._device = dev
        for store, key in zip(self._det, ("boxes", "scores", "labels")):
            store.append(torch.cat([p[key] for p in preds]))
        for store, key in zip(self._gt, ("boxes", "labels")):
            store.append(torch.cat([t[key] for t in target]))
        self._n_det += [p["boxes"].shape[0] for p in preds]
        self._n_gt += [t["boxes"].shape[0] for t in target]

    def _run(self):
        """fp64 [12], fp32 [12] and the int32 classes, on the device of the inputs"""
        dev = self._device
        if not self._n_det:
            dev = dev if dev is not None else torch.device("cpu")
            out = -torch.ones(12, dtype=torch.float64, device=dev)
            return out, out.float(), torch.zeros(0, dtype=torch.int32, device=dev)
        det = [torch.cat(x).contiguous() for x in self._det]
        gt = [torch.cat(x).contiguous() for x in self._gt]
        if _fused_ok(*det, *gt):
            from . import ops
            N, G = det[0].shape[0], gt[0].shape[0]

            def offsets(counts):
                off = [0]
                for n in counts:
                    off.append(off[-1] + n)
                return torch.tensor(off, dtype=torch.int32).to(dev)
            rank, matched, ignored, npig, present, flag = ops.det_map_match(*det, offsets(self._n_det), *gt,
                                                                            offsets(self._n_gt))
            if N and G:
                sorted_idx, seg_off = ops.det_map_order(det[1], det[2], rank)
            else:   # nothing to rank, or nothing to rank against: every class is -1 or scores 0
                sorted_idx = torch.zeros(N, dtype=torch.int32, device=dev)
                seg_off = torch.zeros(257, dtype=torch.int32, device=dev)
            _, out64, out32, outi = ops.det_map_accumulate(sorted_idx, seg_off, rank, matched, ignored, npig, present,
                                                           flag)
            head = outi.cpu()    # the one read-back: class count, flag word, classes
            if int(head[1]) & 1:
                raise ValueError(f"MeanAveragePrecision: a label lies outside [0, {MAP_MAX_LABEL}]")
            if int(head[1]) & 2:
                raise RuntimeError("MeanAveragePrecision: the per-image offsets were refused on the device")
            return out64, out32, outi[2:2 + int(head[0])]
        labels = torch.cat([det[2], gt[1]])
        if labels.numel() and (int(labels.min()) < 0 or int(labels.max()) > MAP_MAX_LABEL):
            raise ValueError(f"MeanAveragePrecision: a label lies outside [0, {MAP_MAX_LABEL}]")
        out64, classes = _map_torch(*det, self._n_det, *gt, self._n_gt, self.iou_thresholds, self.rec_thresholds)
        return out64, out64.float(), torch.tensor(classes, dtype=torch.int32, device=dev)

    def compute_f64(self):
        """the twelve summaries as 0-dim fp64 tensors: what `compute()` rounds to fp32"""
        out64, _, _ = self._run()
        return {k: out64[i] for i, k in enumerate(_MAP_NAMES)}

    def compute(self):
        _, out32, classes = self._run()
        res = {k: out32[i] for i, k in enumerate(_MAP_NAMES)}
        minus = torch.full((), -1.0, dtype=torch.float32, device=out32.device)
        res.update(map_per_class=minus, mar_100_per_class=minus.clone(), classes=classes)
        return res
