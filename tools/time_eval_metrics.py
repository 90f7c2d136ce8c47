#!/usr/bin/env python
"""Cost of the on-device evaluation metrics (ssl4gie_amd.metrics on csrc/metric_ops.hip) beside the reference's
formulation run as torch ops on the same device tensors, its `.item()` calls included — what a driver does without the
kernels.

  seg1      one 224 x 224 logit map against a 1080 x 1350 target (eval_segmentation.py:36-43): device path =
            SegmentationScores.update (counts with the resize inside + scores + accumulator, no read-back); torch-op
            form = F.interpolate to the stored size, then the five metric calls of the loop, each ending in .item()
  seg64     a validation batch of 64 images at 224 x 224, no resize: the same two forms (four metric calls)
  cls40     a 40-batch loader at B = 64, C = 23 (train_classification.py:88-98): device path = 40 x
            ClassificationScores.update(logits) + one scores() + one read-back; torch-op form = argmax, the growing
            concatenation and one re-scoring with .item() per batch
  depth1    one 224 x 224 prediction against a 1080 x 1350 stored depth map (eval_depth.py:43-62): device path =
            DepthErrors.update (no read-back); torch-op form = the loop body with its four .item() calls
  median    lower_median of 1 458 000 values against torch.median on the device

Bytes the device path must touch (`floor_MB`): seg1 the target once (fp32 4 B/pixel; the 200 KB logit map stays in
cache); seg64 logits + targets once; depth1 target_og once + |d / t| written once and read three times by the select's
histogram passes (4 + 4 + 12 B per stored pixel) + the two 224^2 maps; median three reads of the array.  Device time:
HIP events around the call, 10 warm-up + 50 timed repetitions, medians; the torch-op forms end in a read-back, so their
event time includes the waits the host makes.  One JSON line per row; --log FILE appends them:

    timeout 600 python tools/time_eval_metrics.py --log profiles/eval_metrics_timing.log
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def measure(fn, warmup, reps):
    """(median device ms by events, median wall ms) of fn()"""
    ms, wall = [], []
    for it in range(warmup + reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if it >= warmup:
            ms.append(e0.elapsed_time(e1))
            wall.append((t1 - t0) * 1e3)
    return statistics.median(ms), statistics.median(wall)


# ---- the reference's formulation, as torch ops on device tensors (Binary_segmentation/Metrics/performance.py) --------
def _seg_ref(kind, logits, targets, smooth=1e-8):
    num = targets.size(0)
    probs = torch.sigmoid(logits)
    m1 = probs.view(num, -1) > 0.5
    m2 = targets.view(num, -1) > 0.5
    intersection = m1 * m2
    if kind == "dice":
        score = 2.0 * (intersection.sum(1) + smooth) / (m1.sum(1) + m2.sum(1) + smooth)
    elif kind == "iou":
        score = (intersection.sum(1) + smooth) / (m1.sum(1) + m2.sum(1) - intersection.sum(1) + smooth)
    elif kind == "prec":
        score = (intersection.sum(1) + smooth) / (m1.sum(1) + smooth)
    else:
        score = (intersection.sum(1) + smooth) / (m2.sum(1) + smooth)
    return score.sum() / num


def _cls_ref(preds, targets, n_class, smooth=1e-8):
    score = 0
    for i in range(n_class):
        m1 = preds == i
        m2 = targets == i
        intersection = m1 * m2
        score += 2.0 * (intersection.sum() + smooth) / (m1.sum() + m2.sum() + smooth)
    return score / n_class


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()

    from ssl4gie_amd import _lib, metrics
    from ssl4gie_amd.losses import compute_scale_and_shift
    _lib.load()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    rows = []

    def emit(r):
        rows.append(r)
        print(json.dumps(r), flush=True)

    def row(shape, what, fn, floor_bytes=None):
        d, w = measure(fn, a.warmup, a.reps)
        r = {"shape": shape, "what": what, "device_ms": round(d, 4), "wall_ms": round(w, 4)}
        if floor_bytes:
            r.update(floor_MB=round(floor_bytes / 1e6, 2), GB_per_s_of_floor_bytes=round(floor_bytes / (d * 1e-3) / 1e9, 1))
        emit(r)
        return d

    emit({"device": torch.cuda.get_device_name(0), "warmup": a.warmup, "reps": a.reps})
    H, W = 1080, 1350

    # ---- seg1
    logits = 3 * torch.randn(1, 1, 224, 224, device=dev, generator=g)
    target = (torch.rand(1, 1, H, W, device=dev, generator=g) < 0.4).float()
    acc = metrics.SegmentationScores()

    def seg1_ref():
        out = F.interpolate(logits, size=(H, W), mode="bilinear", align_corners=False)
        vals = [_seg_ref(k, out, target).item() for k in ("dice", "iou", "prec", "rec")]
        vals.append(_seg_ref("dice", out, target).item())     # dice_per_instance: the fifth call of the loop
        return vals

    d = row("seg1", "device path: SegmentationScores.update, resize inside, no read-back", lambda: acc.update(logits, target),
            4.0 * H * W + 4.0 * 224 * 224)
    t = row("seg1", "torch ops: F.interpolate + five metric calls, each with .item()", seg1_ref)
    emit({"shape": "seg1", "torch_over_device": round(t / d, 2)})

    # ---- seg64
    logits64 = 3 * torch.randn(64, 1, 224, 224, device=dev, generator=g)
    target64 = (torch.rand(64, 1, 224, 224, device=dev, generator=g) < 0.4).float()
    d = row("seg64", "device path: SegmentationScores.update, no read-back", lambda: acc.update(logits64, target64),
            8.0 * 64 * 224 * 224)
    t = row("seg64", "torch ops: four metric calls, each with .item()",
            lambda: [_seg_ref(k, logits64, target64).item() for k in ("dice", "iou", "prec", "rec")])
    emit({"shape": "seg64", "torch_over_device": round(t / d, 2)})

    # ---- cls40
    C, B, nb = 23, 64, 40
    batches = [(torch.randn(B, C, device=dev, generator=g), torch.randint(0, C, (B,), device=dev, generator=g))
               for _ in range(nb)]

    def cls_dev():
        cs = metrics.ClassificationScores(C)
        for x, tg in batches:
            cs.update(x, tg)
        return cs.scores()[0].item()

    def cls_ref():
        for i, (x, tg) in enumerate(batches):
            if i == 0:
                pred, targ = torch.argmax(x, 1), tg
            else:
                pred, targ = torch.cat((pred, torch.argmax(x, 1)), 0), torch.cat((targ, tg), 0)
            perf = _cls_ref(pred, targ, C).item()
        return perf

    d = row("cls40", "device path: 40 x ClassificationScores.update(logits) + scores() + one read-back", cls_dev)
    t = row("cls40", "torch ops: argmax, concatenate and re-score with .item() at every batch", cls_ref)
    emit({"shape": "cls40", "torch_over_device": round(t / d, 2)})

    # ---- depth1
    og = 0.05 + 0.9 * torch.rand(1, 1, H, W, device=dev, generator=g)
    og[torch.rand(1, 1, H, W, device=dev, generator=g) < 0.25] = 0
    tgt = F.interpolate(og, size=(224, 224), mode="bilinear", align_corners=False)
    pred = (tgt - 0.1) / 0.8 + 0.02 * torch.randn(1, 1, 224, 224, device=dev, generator=g)
    de = metrics.DepthErrors(scale=10.0)

    def depth_ref():
        target = tgt.squeeze(1)
        target_og = og.clone()
        output = pred.squeeze(1)
        scale, shift = compute_scale_and_shift(output, target, target > 0.0)
        output = scale.view(-1, 1, 1) * output + shift.view(-1, 1, 1)
        h, w = target_og.shape[2], target_og.shape[3]
        max_size = max(h, w)
        output = F.interpolate(output.unsqueeze(1), size=(max_size, max_size), mode="bilinear", align_corners=False)
        top, left = metrics.crop_offset(max_size, h), metrics.crop_offset(max_size, w)
        output = output[..., top:top + h, left:left + w]
        output[output < 0.0] = 0.0
        output[output > 1.0] = 1.0
        output[target_og == 0.0] = 0.0
        output *= 10
        target_og *= 10
        r = torch.sqrt(torch.mean((output - target_og)[target_og > 0] ** 2)).item()
        m = torch.median(torch.abs((output - target_og) / target_og)[target_og > 0]).item()
        ab = torch.mean(torch.abs(output - target_og)[target_og > 0]).item()
        r2 = torch.sqrt(torch.mean((output - target_og)[target_og > 0] ** 2)).item()   # rmse_per_instance
        return r, m, ab, r2

    d = row("depth1", "device path: DepthErrors.update, no read-back", lambda: de.update(pred, tgt, og),
            20.0 * H * W + 8.0 * 224 * 224)
    t = row("depth1", "torch ops: eval_depth.py:43-62 with its four .item() calls", depth_ref)
    emit({"shape": "depth1", "torch_over_device": round(t / d, 2)})

    # ---- median
    x = torch.rand(H * W, device=dev, generator=g)
    d = row("median", "device path: lower_median (radix select)", lambda: metrics.lower_median(x), 12.0 * H * W)
    t = row("median", "torch ops: torch.median", lambda: torch.median(x))
    emit({"shape": "median", "torch_over_device": round(t / d, 2)})

    if a.log:
        with open(a.log, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
