#!/usr/bin/env python
"""Cost of the on-device detection input pipeline (ssl4gie_amd.data.DetectionTransform: ops.det_color ->
ops.det_geometry, ops.det_boxes) per batch of 4 at F = 1024 over a ragged bank of Kvasir-like stored sizes (487 x 332
up to 1072 x 1920), split into its stages, beside the same rule written in torch ops as a per-image loop on the same
device tensors — what a user would write without the kernels.

  --part fused   a. parameter draw (torch ops); b. det_color on the recipe's draws; b0. det_color, jitter alone; b2.
                 det_color with sigma = 2 on every sample; c. det_geometry from the scratch; c2. det_geometry from the
                 uint8 bank (the eval path); d. det_boxes; e. the whole DetectionTransform call; e2. the eval transform
  --part torch   t. per image: uint8 -> float / 255, the four jitter ops in the drawn order, reflect pad + two depthwise
                 conv2d passes of 25 taps, rot90 / flips, F.pad + F.interpolate(bicubic, antialias) when a side exceeds
                 F, F.pad to F x F, the boxes' arithmetic on the device; torch.stack of the batch.  The jitter and blur
                 parameters are host numbers drawn beforehand, so the loop never reads the device back.
                 t2. the same loop without the colour stage (the eval path)

Byte floor of a batch (--part fused prints it per row): the colour stage reads 3 B and writes 12 B per stored pixel (the
statistics pass reads 3 B more); the geometry stage reads 12 B per stored pixel and writes 12 B per output pixel.
Device time: HIP events around the call, batches in rotation over a bank larger than the Infinity Cache, 10 warm-up +
50 timed repetitions, medians.  One JSON line per row; --log FILE appends them.  Run each part as a process of its
own, under a time limit:

    timeout 300 python tools/time_det_loader.py --part fused --log profiles/det_loader_timing.log
"""
import argparse
import json
import os
import random
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = ((1072, 1920), (487, 332), (576, 720), (1024, 1280), (1080, 1350), (530, 622))


def measure(fn, warmup, reps):
    ms = []
    for it in range(warmup + reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(it)
        e1.record()
        torch.cuda.synchronize()
        if it >= warmup:
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


# ---- the rule in torch ops, one image at a time ---------------------------------------------------------------------
def gray(x):
    return 0.299 * x[0:1] + 0.587 * x[1:2] + 0.114 * x[2:3]


def blend(a, d, f):
    return (f * a + (1.0 - f) * d).clamp(0.0, 1.0)


def hue_shift(x, f):
    """torchvision's _rgb2hsv / _hsv2rgb"""
    r, g, b = x[0], x[1], x[2]
    maxc, minc = x.max(dim=0).values, x.min(dim=0).values
    eqc = maxc == minc
    cr = maxc - minc
    ones = torch.ones_like(maxc)
    s = cr / torch.where(eqc, ones, maxc)
    div = torch.where(eqc, ones, cr)
    rc, gc, bc = (maxc - r) / div, (maxc - g) / div, (maxc - b) / div
    hr = (maxc == r) * (bc - gc)
    hg = ((maxc == g) & (maxc != r)) * (2.0 + rc - bc)
    hb = ((maxc != g) & (maxc != r)) * (4.0 + gc - rc)
    h = torch.fmod((hr + hg + hb) / 6.0 + 1.0, 1.0)
    h = torch.remainder(h + f, 1.0)
    i = torch.floor(h * 6.0)
    fr = h * 6.0 - i
    i = i.to(torch.int64) % 6
    p = (maxc * (1.0 - s)).clamp(0.0, 1.0)
    q = (maxc * (1.0 - fr * s)).clamp(0.0, 1.0)
    t = (maxc * (1.0 - (1.0 - fr) * s)).clamp(0.0, 1.0)
    v = maxc
    table = torch.stack([torch.stack([v, q, p, p, t, v]), torch.stack([t, v, v, q, p, p]), torch.stack([p, p, t, v, v, q])])
    return table.gather(1, i.expand(3, 1, *i.shape)).squeeze(1)


def torch_image(u8_hwc, boxes, p, Fx, color):
    """p: host dict of one sample's draws"""
    x = u8_hwc.permute(2, 0, 1).to(torch.float32).div(255)
    if color:
        for op in p["order"]:
            f = p["factors"][op]
            x = blend(x, 0.0, f) if op == 0 else blend(x, gray(x).mean(), f) if op == 1 else blend(x, gray(x), f) if op == 2 \
                else hue_shift(x, f)
        k = torch.arange(-12, 13, device=x.device, dtype=torch.float32)
        w = torch.exp(-0.5 * (k / p["sigma"]) ** 2)
        w = (w / w.sum()).view(1, 1, 25).expand(3, 1, 25)
        y = F.pad(x.unsqueeze(0), (12, 12, 12, 12), mode="reflect")
        x = F.conv2d(F.conv2d(y, w.unsqueeze(2), groups=3), w.unsqueeze(3), groups=3)[0]
    H, W = x.shape[1:]
    b = boxes.clone()
    if p["r"]:
        x = torch.rot90(x, dims=[1, 2])
        b = torch.stack([b[:, 1], W - b[:, 2], b[:, 3], W - b[:, 0]], dim=1)
        H, W = W, H
    if p["h"]:
        x = x.flip(-1)
        b = torch.stack([W - b[:, 2], b[:, 1], W - b[:, 0], b[:, 3]], dim=1)
    if p["v"]:
        x = x.flip(-2)
        b = torch.stack([b[:, 0], H - b[:, 3], b[:, 2], H - b[:, 1]], dim=1)
    if H > Fx or W > Fx:
        x = F.pad(x, (0, W % 2, 0, H % 2))
        H, W = H + H % 2, W + W % 2
        x = F.interpolate(x.unsqueeze(0), size=(H // 2, W // 2), mode="bicubic", antialias=True, align_corners=False)[0]
        H, W = H // 2, W // 2
        b = b / 2
    p1, p2 = (Fx - W) // 2, (Fx - H) // 2
    x = F.pad(x, (p1, Fx - W - p1, p2, Fx - H - p2))
    return x, b + torch.tensor([p1, p2, p1, p2], dtype=torch.float32, device=b.device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("fused", "torch"), required=True)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--fixed-size", type=int, default=1024)
    ap.add_argument("--bank", type=int, default=120, help="images in the bank (about 2.9 MB each: 344 MB, beyond the Infinity Cache)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()

    from ssl4gie_amd import _lib, ops
    from ssl4gie_amd.data import DetectionTransform, RaggedImageBank
    _lib.load()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, Fx, n = a.batch, a.fixed_size, a.bank
    rows = []

    def emit(r):
        r = {"part": a.part, **r}
        rows.append(r)
        print(json.dumps(r), flush=True)

    g = torch.Generator(device=dev).manual_seed(0)
    sizes = np.array([SIZES[i % len(SIZES)] for i in range(n)], dtype=np.int32)
    _, total = RaggedImageBank.offsets_of(sizes)
    pixels = torch.randint(0, 256, (total,), dtype=torch.uint8, device=dev, generator=g)
    boxes = torch.tensor([[0.1 * w, 0.2 * h, 0.7 * w, 0.9 * h] for h, w in sizes.tolist()], dtype=torch.float32)
    bank = RaggedImageBank(pixels, torch.from_numpy(sizes), boxes.to(dev), torch.arange(n + 1, dtype=torch.int64).to(dev))
    tf = DetectionTransform(Fx, generator=g)
    ev = DetectionTransform.eval(Fx)
    n_sets = a.warmup + a.reps
    rng = random.Random(0)
    idx_host = [[rng.randrange(n) for _ in range(B)] for _ in range(n_sets)]
    index = [torch.tensor(i, dtype=torch.int64, device=dev) for i in idx_host]
    sets = [tf.draw(B, dev) for _ in range(n_sets)]
    stored = [sum(bank.sizes_host[i][0] * bank.sizes_host[i][1] for i in ih) for ih in idx_host]
    emit({"batch": B, "fixed_size": Fx, "bank_images": n, "bank_MB": round(total / 1e6, 1), "stored_sizes": list(SIZES),
          "mean_stored_pixels_per_batch": round(statistics.mean(stored)), "warmup": a.warmup, "reps": a.reps,
          "device": torch.cuda.get_device_name(0)})

    def row(what, fn, floor_bytes=None, **extra):
        d, lo, hi = measure(fn, a.warmup, a.reps)
        r = {"what": what, "device_ms": round(d, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4)}
        if floor_bytes:
            r.update(floor_MB=round(floor_bytes / 1e6, 1), TB_per_s_of_floor_bytes=round(floor_bytes / (d * 1e-3) / 1e12, 3))
        r.update(extra)
        emit(r)
        return d

    mean_px, out_px = statistics.mean(stored), float(B * Fx * Fx)
    if a.part == "fused":
        scratch = torch.empty(B, 3, (bank.max_pixels + 3) & ~3, dtype=torch.float32, device=dev)
        max_hw = lambda it: (max(bank.sizes_host[i][0] for i in idx_host[it]), max(bank.sizes_host[i][1] for i in idx_host[it]))
        color = lambda it, sigma=None: ops.det_color(bank.pixels, bank.offsets, bank.sizes, index[it], sets[it][0], sets[it][1],
                                                     sets[it][2] if sigma is None else sigma, max_hw(it), scratch)
        geo = lambda it, s=scratch: ops.det_geometry(bank.pixels, bank.offsets, bank.sizes, index[it], sets[it][3], Fx,
                                                     tf.mean, tf.std, s)
        starts = torch.arange(B + 1, dtype=torch.int64, device=dev)
        row("a. drawing one batch's parameters (torch ops)", lambda it: tf.draw(B, dev))
        zero, two = torch.zeros(B, device=dev), torch.full((B,), 2.0, device=dev)
        row("b0. det_color, jitter alone (sigma = 0 on every sample)", lambda it: color(it, zero), 18.0 * mean_px)
        row("b. det_color, the loader's recipe (sigma in [0.001, 2])", color, 18.0 * mean_px)
        row("b2. det_color, sigma = 2 on every sample", lambda it: color(it, two), 18.0 * mean_px)
        row("c. det_geometry from the fp32 scratch", geo, 12.0 * mean_px + 12.0 * out_px)
        row("c2. det_geometry from the uint8 bank (eval path)", lambda it: geo(it, None), 3.0 * mean_px + 12.0 * out_px)
        row("d. det_boxes", lambda it: ops.det_boxes(bank.boxes, bank.box_labels, bank.box_offsets, bank.sizes, index[it],
                                                     sets[it][3], starts, B, 1, Fx))
        row("e. DetectionTransform()(bank, index): a + b + c + d and the split points' copy",
            lambda it: tf(bank, index[it], idx_host[it]))
        row("e2. DetectionTransform.eval()(bank, index)", lambda it: ev(bank, index[it], idx_host[it]))
    else:
        host = []
        for it in range(n_sets):
            f, o, s, gm = (t.cpu().tolist() for t in sets[it])
            host.append([dict(factors=f[b], order=o[b], sigma=max(s[b], 1e-6), r=bool(gm[b] & 4), h=bool(gm[b] & 1),
                              v=bool(gm[b] & 2)) for b in range(B)])

        def loop(it, color=True):
            out = [torch_image(bank.image(i), bank.boxes[i:i + 1], host[it][b], Fx, color) for b, i in enumerate(idx_host[it])]
            return torch.stack([o[0] for o in out]), [o[1] for o in out]

        row("t. torch ops, per-image loop: jitter + 25-tap blur + rot90 / flips + antialiased halving + pad + boxes", loop)
        row("t2. torch ops, per-image loop without the colour stage (eval path)", lambda it: loop(it, False))
    if a.log:
        with open(a.log, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
