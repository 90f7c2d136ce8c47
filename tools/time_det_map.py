#!/usr/bin/env python
"""Cost of the on-device detection metric (ssl4gie_amd.metrics.MeanAveragePrecision.compute() on
csrc/det_map_ops.hip) beside the torch formulation of the same file run on the same device tensors
(SSL4GIE_FUSED_METRICS=0: torch ops in pycocotools' order of steps, with the host control flow and read-backs that
takes) — what a driver gets without the kernels.  torchmetrics itself (absent here) moves everything to the host.

  kvasir    100 images, 100 detections each, 1-3 boxes, 1 class: a validation pass of train_detection.py
  coco      5000 images, 100 detections each, ~7 boxes, 80 classes: COCO val2017's size

`update` is outside the timed region (it is five torch.cat per batch on either path); the timed call is compute(): the
concatenation of the stored batches, the offsets' upload, match + order + accumulate (1 + 15 + 2 launches, 3 memsets)
and the one read-back.  Device time: HIP events around the call, medians; wall time beside it.  The torch formulation
is timed the same way, after one untimed run that yields its values, over `reps` runs as its row reports them: 3 at the
kvasir size (--torch-reps), one at the coco size, where a run takes minutes (--torch-reps-coco).  One JSON line per
row; --log FILE appends them:

    timeout 900 python tools/time_det_map.py --log profiles/det_map_timing.log
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

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


def make_case(rng, n_img, n_det, box_counts, n_class, stray):
    """per image: ground truths of a few classes, detections = perturbed copies of them (a share `stray` with a random
    label and place), scores in (0, 1)"""
    preds, target = [], []
    for _ in range(n_img):
        g = int(rng.choice(box_counts))
        side = rng.uniform(12, 260, (g, 2))
        xy = rng.uniform(0, 640 - side)
        gb = np.concatenate([xy, xy + side], 1).astype(np.float32)
        gl = rng.choice(rng.integers(0, n_class, 3), g).astype(np.int64)
        src = rng.integers(0, g, n_det)
        wh = np.tile(side[src], 2)
        db = (gb[src] + rng.uniform(-0.3, 0.3, (n_det, 4)) * wh * rng.random((n_det, 1))).astype(np.float32)
        dl = gl[src].copy()
        far = rng.random(n_det) < stray
        dl[far] = rng.integers(0, n_class, int(far.sum()))
        preds.append({"boxes": torch.from_numpy(db), "scores": torch.from_numpy(rng.random(n_det).astype(np.float32)),
                      "labels": torch.from_numpy(dl)})
        target.append({"boxes": torch.from_numpy(gb), "labels": torch.from_numpy(gl)})
    return preds, target


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--torch-reps-coco", type=int, default=1)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()

    from ssl4gie_amd import _lib, metrics
    _lib.load()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rows = []

    def emit(r):
        rows.append(r)
        print(json.dumps(r), flush=True)

    emit({"device": torch.cuda.get_device_name(0), "warmup": a.warmup, "reps": a.reps})
    sizes = (("kvasir", 100, 100, (1, 2, 3), 1, 0.2, a.torch_reps), ("coco", 5000, 100, (3, 5, 7, 9, 11), 80, 0.15,
                                                                      a.torch_reps_coco))
    for name, n_img, n_det, box_counts, n_class, stray, torch_reps in sizes:
        preds, target = make_case(np.random.default_rng(0), n_img, n_det, box_counts, n_class, stray)
        preds = [{k: v.to(dev) for k, v in p.items()} for p in preds]
        target = [{k: v.to(dev) for k, v in t.items()} for t in target]
        m = metrics.MeanAveragePrecision()
        for s in range(0, n_img, a.batch):
            m.update(preds[s:s + a.batch], target[s:s + a.batch])
        shape = {"shape": name, "images": n_img, "detections": n_img * n_det,
                 "ground_truths": sum(t["boxes"].shape[0] for t in target), "classes": n_class}
        os.environ["SSL4GIE_FUSED_METRICS"] = "1"
        fused = m.compute_f64()
        d, w = measure(m.compute, a.warmup, a.reps)
        emit({**shape, "what": "device path: compute() = match + order + accumulate + one read-back",
              "device_ms": round(d, 4), "wall_ms": round(w, 4), "map": float(fused["map"])})
        os.environ["SSL4GIE_FUSED_METRICS"] = "0"
        plain = m.compute_f64()     # the values, untimed
        dev_t, wall_t = measure(m.compute, 0, torch_reps)
        os.environ["SSL4GIE_FUSED_METRICS"] = "1"
        emit({**shape, "what": "torch formulation on the same device tensors", "device_ms": round(dev_t, 2),
              "wall_ms": round(wall_t, 2), "reps": torch_reps, "map": float(plain["map"]),
              "max_abs_diff_of_the_twelve": max(abs(float(plain[k]) - float(fused[k])) for k in fused)})
        emit({"shape": name, "torch_over_device": round(dev_t / d, 1)})

    if a.log:
        with open(a.log, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
