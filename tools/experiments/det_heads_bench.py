#!/usr/bin/env python
"""Cost of the Faster R-CNN heads (ssl4gie_amd/Models/detection.py on csrc/det_head_ops.hip) beside the torch
formulations of the same file (SSL4GIE_FUSED_DET_HEADS=0) on the same device tensors, at the reference's size:
F = 1024, B = 4, num_classes = 2, ViT-B backbone, bf16 operands.

  proposals     rpn_proposals: top-k per level, decode, NMS per (image, level), the first post_nms_top_n (training counts)
  roi_align     forward and backward at 2048 RoIs over the four pyramid maps
  postprocess   decode, NMS per (image, class), the first 100 (eval counts)
  train / eval  the whole forward (train: with the four losses; the backward is not part of this row)

Device time by HIP events around `inner` back-to-back calls (20 for the kernel stages, so that a timed window is several
milliseconds, 2 for the whole model), divided by `inner`; medians over --reps windows (30), wall time beside it; every
shape is warmed up first.  The kernel path is timed before AND after the torch formulation (`device_ms`,
`device_ms_again`): the spread between the two is the noise of the box.  The torch formulation is timed one call per
window over --torch-reps windows (5); its NMS sweeps on the host, as torchvision's CUDA nms does, so its rows are mostly
host time.  One JSON line per row; --log FILE appends the rows gathered.  Nothing is caught: the first exception (a HIP
error among them) ends the process with a non-zero status after the rows gathered so far are written, and nothing more
is started on the device:

    timeout -k 10 900 python tools/experiments/det_heads_bench.py --log profiles/det_heads_timing.log
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def measure(fn, warmup, reps, inner=1, setup=None):
    """(median device ms by events, median wall ms) of one fn(); a window holds `inner` calls; setup() runs untimed
    before every window"""
    ms, wall = [], []
    for it in range(warmup + reps):
        if setup is not None:
            setup()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if it >= warmup:
            ms.append(e0.elapsed_time(e1) / inner)
            wall.append((t1 - t0) * 1e3 / inner)
    return statistics.median(ms), statistics.median(wall)


def recording(cls):
    """the detector with the outputs of its stages kept from the last forward (the stages' inputs below)"""

    class Recording(cls):
        recording = False

        def rpn_head(self, features):
            heads, grids = super().rpn_head(features)
            if self.recording:
                self.last = dict(features=features, heads=heads, grids=grids)
            return heads, grids

        def rpn_proposals(self, heads, grids, B, F):
            r = super().rpn_proposals(heads, grids, B, F)
            if self.recording:
                self.last.update(props=r[0], ok=r[1])
            return r

        def box_head(self, features, rois, roi_batch, F):
            out = super().box_head(features, rois, roi_batch, F)
            if self.recording:
                self.last["out"] = out
            return out

    return Recording


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--rois", type=int, default=2048)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--torch-reps", type=int, default=5)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    rows = []
    try:
        run(a, rows)
    finally:   # whatever ended the run, the rows measured so far are kept; an exception goes on to end the process
        if a.log:
            with open(a.log, "a") as f:
                for r in rows:
                    f.write(json.dumps(r) + "\n")


def run(a, rows):
    from ssl4gie_amd import _lib, ops
    from ssl4gie_amd.Models import detection as det, models
    _lib.load()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    F, B = a.size, a.batch

    def emit(r):
        rows.append(r)
        print(json.dumps(r), flush=True)

    def stage(name, fused, plain, inner, check=None, extra=None):
        """fused / plain: callables; check(): agreement figures for the row; extra(): further timings for it"""
        try:
            os.environ["SSL4GIE_FUSED_DET_HEADS"] = "1"
            d0, w0 = measure(fused, a.warmup, a.reps, inner)
            os.environ["SSL4GIE_FUSED_DET_HEADS"] = "0"
            dt, wt = measure(plain, 1, a.torch_reps)
            os.environ["SSL4GIE_FUSED_DET_HEADS"] = "1"
            d1, w1 = measure(fused, 1, a.reps, inner)
        finally:
            os.environ["SSL4GIE_FUSED_DET_HEADS"] = "1"
        r = {"stage": name, "device_ms": round(d0, 4), "wall_ms": round(w0, 4), "device_ms_again": round(d1, 4),
             "calls_per_window": inner, "torch_device_ms": round(dt, 3), "torch_wall_ms": round(wt, 3),
             "torch_reps": a.torch_reps, "torch_over_device": round(dt / max(d0, d1), 2)}
        if check is not None:
            r.update(check())
        if extra is not None:
            r.update(extra())
        emit(r)

    torch.manual_seed(0)
    backbone = models.VisionTransformer_from_Any(False, 0, False, None, True, F, 768, 12, 12, "cls")
    m = recording(det.FasterRCNN)(backbone, num_classes=2, image_mean=[0.485, 0.456, 0.406], image_std=[0.229, 0.224, 0.225])
    m.transform.fixed_size = (F, F)
    with torch.no_grad():   # heads that decide something (the 0.01 initialisation leaves every score at 0.5)
        g = torch.Generator().manual_seed(1)
        for p in list(m.rpn.parameters()) + list(m.roi_heads.box_predictor.parameters()):
            p.copy_(torch.randn(p.shape, generator=g) * (0.05 if p.dim() > 1 else 0.2))
    m.to(dev).set_precision(a.precision)
    g = torch.Generator().manual_seed(2)
    images = list(torch.rand(B, 3, F, F, generator=g).to(dev).unbind(0))
    targets = []
    for b in range(B):
        k = 1 + b % 3
        xy = torch.rand(k, 2, generator=g) * F * 0.5
        wh = torch.rand(k, 2, generator=g) * F * 0.35 + 40
        targets.append({"boxes": torch.cat([xy, xy + wh], 1).to(dev), "labels": torch.ones(k, dtype=torch.int64, device=dev)})
    emit({"device": torch.cuda.get_device_name(0), "F": F, "B": B, "num_classes": 2, "precision": a.precision,
          "rois": a.rois, "warmup": a.warmup, "reps": a.reps, "torch_reps": a.torch_reps})

    # the stages' inputs: one training forward and one eval forward of the engine
    m.recording = True
    m.train()
    with torch.no_grad():
        m(images, targets)
    Lt = m.last
    m.recording = False
    heads, grids = [h.detach() for h in Lt["heads"]], Lt["grids"]
    maps = [Lt["features"][k].detach() for k in ("0", "1", "2", "3")]
    scales = [2.0 ** round(math.log2(x.shape[2] / F)) for x in maps]

    m.train()
    stage("proposals (train counts: 2000 per level, 2000 per image)",
          lambda: m.rpn_proposals(heads, grids, B, F), lambda: m.rpn_proposals(heads, grids, B, F), 20)

    props = Lt["props"].reshape(-1, 4)
    n = a.rois
    rois = props[torch.arange(n, device=dev) % props.shape[0]].contiguous()
    rb = (torch.arange(n, device=dev) * B // n).to(torch.int32)
    dt = m.dtype_
    stage(f"roi_align forward, {n} RoIs",
          lambda: ops.roi_align_fwd(maps, scales, rois, rb, dt), lambda: det.roi_align_torch(maps, scales, rois, rb, dt), 20,
          lambda: {"max_abs_diff": float((ops.roi_align_fwd(maps, scales, rois, rb, torch.float32) -
                                          det.roi_align_torch(maps, scales, rois, rb)).abs().max())})
    dy = torch.randn(n, maps[0].shape[1] * 49, device=dev).to(dt)
    dm = [torch.zeros(x.shape[0], x.shape[2], x.shape[3], x.shape[1], device=dev).permute(0, 3, 1, 2) for x in maps]

    def bwd_fused():
        for t in dm:
            t.zero_()
        ops.roi_align_bwd(dm, scales, rois, rb, dy)

    leaf = [x.clone().requires_grad_(True) for x in maps]

    def bwd_plain():
        for t in leaf:
            t.grad = None
        det.roi_align_torch(leaf, scales, rois, rb, dt).backward(dy)

    graph = {}

    def bwd_only_setup():
        for t in leaf:
            t.grad = None
        graph["y"] = det.roi_align_torch(leaf, scales, rois, rb, dt)

    def bwd_only():   # the backward of the torch formulation alone: its forward is built, untimed, before each window
        d, _ = measure(lambda: graph["y"].backward(dy), 1, a.torch_reps, 1, bwd_only_setup)
        return {"torch_backward_only_device_ms": round(d, 3)}

    stage(f"roi_align backward, {n} RoIs (fused: zeroing the four maps + the adds; torch: forward + backward)",
          bwd_fused, bwd_plain, 20, extra=bwd_only)

    m.eval()
    m.recording = True
    with torch.no_grad():
        m(images)
    Le = m.last
    m.recording = False
    out, eprops, eok = Le["out"].float(), Le["props"], Le["ok"]
    stage("postprocess (eval: 1000 proposals per image, 100 detections)",
          lambda: m.postprocess(out, eprops, eok, F), lambda: m.postprocess(out, eprops, eok, F), 20)


    def fwd_eval():
        with torch.no_grad():
            m(images)

    stage("eval forward, whole model", fwd_eval, fwd_eval, 2)
    m.train()

    def fwd_train():
        with torch.no_grad():
            m(images, targets)

    stage("train forward, whole model (no backward)", fwd_train, fwd_train, 2)


if __name__ == "__main__":
    main()
