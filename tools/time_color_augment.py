#!/usr/bin/env python
"""Cost of the on-device colour stage (ssl4gie_amd.data.ColorAugment -> ops.color_augment) at the MoCo-v3 batch:
B = 256, S = 224, fp32 [0, 1] images in, normalised fp32 out.

  (a) the view-1 recipe (jitter p 0.8, grayscale p 0.2, blur p 1.0, sigma in [0.1, 2]);
  (b) the view-2 recipe (blur p 0.1, solarize p 0.2);
  (c) the statistics pass alone: the launch pair with contrast as the only op on every sample, minus the pair with
      nothing switched on (its statistics workgroups exit at once); the apply kernel takes its pointwise path in both;
  (d) the view-1 recipe with one sigma on every sample, radius by radius.

Byte floor per view: the statistics pass reads the samples that carry a contrast op (0.8 of 154 MB on average), the
apply kernel reads 154 MB and writes 154 MB.  Reported: device time, TB/s of that floor, and the share of the 55 ms
MoCo-R50 step.  The goal to report against: two views under 2 % of the step.

Device time: HIP events around the call.  Every launch gets an input batch of its own (16 batches of 154 MB in
rotation, 2.5 GB: ten times the 256 MiB Infinity Cache) and freshly drawn parameters; the parameter draw is timed
separately.  10 warm-up + 50 timed repetitions, medians.  One JSON line per row; --log FILE appends them to a file.

    python tools/time_color_augment.py --log profiles/color_augment_timing.log
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MOCO_STEP_MS = 55.0


def measure(fn, warmup, reps):
    dev_ms = []
    for it in range(warmup + reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(it)
        e1.record()
        torch.cuda.synchronize()
        if it >= warmup:
            dev_ms.append(e0.elapsed_time(e1))
    return statistics.median(dev_ms), min(dev_ms), max(dev_ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--pool", type=int, default=16, help="input batches in rotation")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()

    from ssl4gie_amd import _lib, ops
    from ssl4gie_amd.data import ColorAugment
    _lib.load()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, S = a.batch, a.size
    rows = []

    def emit(r):
        rows.append(r)
        print(json.dumps(r), flush=True)

    g = torch.Generator(device=dev).manual_seed(0)
    pool = [torch.rand(B, 3, S, S, device=dev, generator=g) for _ in range(a.pool)]
    out = torch.empty_like(pool[0])
    image_bytes = 12.0 * S * S * B
    emit({"batch": B, "size": S, "image_MB": round(image_bytes / 1e6, 1), "pool_batches": a.pool, "warmup": a.warmup,
          "reps": a.reps, "device": torch.cuda.get_device_name(0)})
    n_sets = a.warmup + a.reps

    def timed(what, tf, extra=None):
        sets = [tf.draw(B, dev) for _ in range(n_sets)]
        with_contrast = statistics.mean(float((s[1] == 1).any(dim=1).double().mean()) for s in sets[a.warmup:])
        floor_bytes = (2.0 + with_contrast) * image_bytes
        d, lo, hi = measure(lambda it: ops.color_augment(pool[it % a.pool], *sets[it], tf.mean, tf.std, out=out),
                            a.warmup, a.reps)
        r = {"what": what, "device_ms": round(d, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4),
             "samples_with_contrast": round(with_contrast, 3), "floor_MB": round(floor_bytes / 1e6, 1),
             "TB_per_s_of_floor_bytes": round(floor_bytes / (d * 1e-3) / 1e12, 3),
             "fraction_of_8TBps": round(floor_bytes / (d * 1e-3) / 8e12, 3),
             "share_of_55ms_moco_step": round(d / MOCO_STEP_MS, 5)}
        r.update(extra or {})
        emit(r)
        return d

    v1 = ColorAugment(blur_p=1.0, solarize_p=0.0, generator=g)
    v2 = ColorAugment(blur_p=0.1, solarize_p=0.2, generator=g)
    d1 = timed("a. view 1: jitter 0.8, gray 0.2, blur 1.0", v1)
    d2 = timed("b. view 2: jitter 0.8, gray 0.2, blur 0.1, solarize 0.2", v2)
    emit({"what": "a + b. two views", "device_ms": round(d1 + d2, 4), "share_of_55ms_moco_step": round((d1 + d2) / MOCO_STEP_MS, 5),
          "goal": "under 0.02", "met": bool((d1 + d2) / MOCO_STEP_MS < 0.02)})
    d, _, _ = measure(lambda it: v1.draw(B, dev), a.warmup, a.reps)
    emit({"what": "drawing one view's parameters (torch ops)", "device_ms": round(d, 4)})

    # (c) the statistics pass: contrast alone on every sample against no jitter at all, nothing else switched on
    every = ColorAugment(brightness=0.0, contrast=0.4, saturation=0.0, hue=0.0, jitter_p=1.0, gray_p=0.0, blur_p=0.0, generator=g)
    none = ColorAugment(jitter_p=0.0, gray_p=0.0, blur_p=0.0, generator=g)
    dc = timed("c. contrast alone on every sample (statistics pass + pointwise apply)", every)
    dn = timed("c. nothing switched on (statistics workgroups exit + pointwise apply)", none)
    emit({"what": "c. statistics pass alone (difference of the two)", "device_ms": round(dc - dn, 4),
          "read_MB": round(image_bytes / 1e6, 1), "TB_per_s": round(image_bytes / max(dc - dn, 1e-6) / 1e9, 3)})
    # blur radius by radius, every sample the same sigma
    for sigma in (0.3, 0.6, 1.0, 1.3, 1.6, 2.0):
        fixed = ColorAugment(blur_p=1.0, blur_sigma=(sigma, sigma), generator=g)
        timed(f"d. view-1 recipe, sigma = {sigma} on every sample (R = {math.ceil(3.0 * float(torch.tensor(sigma, dtype=torch.float32)))})", fixed)
    if a.log:
        with open(a.log, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
