#!/usr/bin/env python
"""Cost of the on-device input pipeline (ssl4gie_amd.data) on the MAE ViT-B workload:

  (a) the view sampler alone, B = 256, S = 224, random-resized-crop boxes (scale 0.2 .. 1) out of a 256 x 256 bank,
      bicubic and bilinear: device time per launch, and bytes/s against its byte floor
          sum of the boxes' bytes read + 12 S^2 B bytes written.
      The bank (1536 images, 302 MB) is larger than the 256 MiB Infinity Cache and every launch draws other
      images, so the reads are not served from it.
  (b) the MAE ViT-B training step (forward, backward, ArenaAdamW) fed by DeviceLoader against the same step on one
      resident batch, the two alternating within this one call: ms per step, and the sampler's share.

Device time: HIP events around the call; host time: wall clock from the call to its return.  10 warm-up + 50 timed
repetitions, medians.  One JSON line per row; --log FILE appends them to a file.

    python tools/time_input_pipeline.py --log profiles/input_pipeline_timing.log
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def measure(fn, warmup, reps):
    dev_ms, host_ms = [], []
    for it in range(warmup + reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        fn(it)
        t1 = time.perf_counter()
        e1.record()
        torch.cuda.synchronize()
        if it >= warmup:
            dev_ms.append(e0.elapsed_time(e1))
            host_ms.append(1e3 * (t1 - t0))
    return statistics.median(dev_ms), statistics.median(host_ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--stored", type=int, default=256)
    ap.add_argument("--images", type=int, default=1536)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--skip-step", action="store_true", help="part (a) only")
    ap.add_argument("--log", default=None)
    a = ap.parse_args()

    from ssl4gie_amd import _lib, ops, optim
    from ssl4gie_amd.data import DeviceImageBank, DeviceLoader, RandomResizedCropFlip
    _lib.load()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, S, Hs = a.batch, a.size, a.stored
    rows = []

    def emit(r):
        rows.append(r)
        print(json.dumps(r), flush=True)

    g = torch.Generator(device=dev).manual_seed(0)
    images = torch.randint(0, 256, (a.images, Hs, Hs, 3), dtype=torch.uint8, device=dev, generator=g)
    bank = DeviceImageBank(images)
    emit({"bank": [a.images, Hs, Hs, 3], "bank_MB": round(images.numel() / 1e6, 1), "batch": B, "size": S,
          "warmup": a.warmup, "reps": a.reps, "device": torch.cuda.get_device_name(0)})

    # ---- (a) the sampler alone
    n_sets = a.warmup + a.reps
    for name in ("bicubic", "bilinear"):
        tf = RandomResizedCropFlip(S, scale=(0.2, 1.0), interpolation=name, generator=g)
        sets = []
        for k in range(n_sets):   # other images and other boxes on every launch
            index = torch.randperm(a.images, device=dev, generator=g)[:B].contiguous()
            box, flip = tf.draw(B, Hs, Hs, dev)
            sets.append((index, box, flip))
        box_bytes = statistics.mean(float((s[1][:, 2].double() * s[1][:, 3].double()).sum()) * 3 for s in sets[a.warmup:])
        floor_bytes = box_bytes + 12.0 * S * S * B
        d, h = measure(lambda it: ops.view_sample_u8(images, *sets[it], S, name), a.warmup, a.reps)
        emit({"what": f"a. view_sample_u8 {name}, boxes scale (0.2, 1)", "device_ms": round(d, 4), "host_ms": round(h, 4),
              "floor_MB": round(floor_bytes / 1e6, 1), "box_MB_read": round(box_bytes / 1e6, 1),
              "TB_per_s_of_floor_bytes": round(floor_bytes / (d * 1e-3) / 1e12, 3),
              "fraction_of_8TBps": round(floor_bytes / (d * 1e-3) / 8e12, 3)})
        whole = torch.tensor([[0, 0, Hs, Hs]] * B, dtype=torch.int32, device=dev)
        d, h = measure(lambda it: ops.view_sample_u8(images, sets[it][0], whole, sets[it][2], S, name), a.warmup, a.reps)
        wb = 3.0 * Hs * Hs * B + 12.0 * S * S * B
        emit({"what": f"a. view_sample_u8 {name}, whole-image boxes", "device_ms": round(d, 4), "host_ms": round(h, 4),
              "floor_MB": round(wb / 1e6, 1), "TB_per_s_of_floor_bytes": round(wb / (d * 1e-3) / 1e12, 3)})
        d, h = measure(lambda it: tf.draw(B, Hs, Hs, dev), a.warmup, a.reps)
        emit({"what": "a. drawing boxes and flips (torch ops)", "device_ms": round(d, 4), "host_ms": round(h, 4)})
    if a.skip_step:
        return finish(a, rows)

    # ---- (b) the MAE ViT-B step, loader-fed against one resident batch
    from ssl4gie_amd.Models.mae import models_mae
    torch.manual_seed(0)
    model = models_mae.mae_vit_base_patch16(norm_pix_loss=True).to(dev).set_precision(a.precision)
    opt = optim.ArenaAdamW(model, [p for p in model.parameters() if p.requires_grad], lr=1.5e-4, betas=(0.9, 0.95),
                           weight_decay=0.05)
    tf = RandomResizedCropFlip(S, scale=(0.2, 1.0), generator=g)
    loader = DeviceLoader(bank, B, transform=tf)
    resident = next(iter(loader))[0]

    def step(samples):
        loss, _, _ = model(samples, mask_ratio=0.75)
        loss.backward()
        opt.step()
        opt.zero_grad()

    feed = {"it": iter(loader)}

    def next_batch():
        try:
            return next(feed["it"])[0]
        except StopIteration:
            feed["it"] = iter(loader)
            return next(feed["it"])[0]

    t_res, t_load, t_samp = [], [], []
    for it in range(a.warmup + a.reps):
        for which in ("resident", "loader"):
            torch.cuda.synchronize()
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record()
            samples = resident if which == "resident" else next_batch()
            e1.record()
            step(samples)
            e2.record()
            torch.cuda.synchronize()
            if it >= a.warmup:
                if which == "resident":
                    t_res.append(e0.elapsed_time(e2))
                else:
                    t_load.append(e0.elapsed_time(e2))
                    t_samp.append(e0.elapsed_time(e1))
    r, l, s = statistics.median(t_res), statistics.median(t_load), statistics.median(t_samp)
    emit({"what": "b. MAE ViT-B step, one resident batch", "device_ms": round(r, 3), "img_per_s": round(B / r * 1e3, 1)})
    emit({"what": "b. MAE ViT-B step fed by DeviceLoader", "device_ms": round(l, 3), "img_per_s": round(B / l * 1e3, 1),
          "input_ms": round(s, 4), "input_share_of_resident_step": round(s / r, 4), "slowdown": round(l / r - 1.0, 4)})
    finish(a, rows)


def finish(a, rows):
    if a.log:
        with open(a.log, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
