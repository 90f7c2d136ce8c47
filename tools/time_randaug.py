#!/usr/bin/env python
"""Cost of the on-device input of the MAE fine-tuning recipe (ssl4gie_amd.data.MAEFinetuneTransform: view_sample_u8 ->
quantize_u8 -> randaug_layer x n -> normalize_erase_u8) at B = 256, S = 224, split into its stages, and of the PIL path
it replaces.

  --part gpu   a. the draws (torch ops); b. crop + flip (view_sample_u8); c. quantize_u8; d1 / d2. each RandAugment layer
               on the recipe's draws; d-<op>. a layer with ONE op on every sample, op by op; e. normalize_erase_u8 on
               the recipe's boxes; f. the whole transform call.  Device time: HIP events around the call, 10 warm-up +
               50 timed repetitions on draws made beforehand, medians.
  --part pil   the reference's per-image path on the host CPU (one process, no DataLoader workers): PIL crop +
               bicubic resize + flip, the two RandAugment ops through PIL as timm calls them (drawn by the same
               RandAugment class), ToTensor + Normalize + the erase in numpy.  Host wall time per image.

Byte floor of a layer: the uint8 image read and written once, 6 B per pixel (the histogram ops read it once more).
One JSON line per row; --log FILE appends them.

    timeout 300 python tools/time_randaug.py --part gpu --log profiles/randaug_timing.log
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


def pil_image(img, S, box, flip, ops_row, fill, mean, std, ebox, rs):
    """one image through PIL as transforms_imagenet_train runs it, on parameters that are already drawn"""
    from PIL import Image, ImageEnhance, ImageOps
    top, left, h, w = box
    im = img.crop((left, top, left + w, top + h)).resize((S, S), Image.BICUBIC)
    if flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    kw = dict(resample=Image.BICUBIC, fillcolor=fill)
    for op, arg, m in ops_row:
        if op == 0:
            im = ImageOps.autocontrast(im)
        elif op == 1:
            im = ImageOps.equalize(im)
        elif op == 2:
            im = ImageOps.invert(im)
        elif op == 3:
            im = im.rotate(arg, **kw)
        elif op == 4:
            im = im if int(arg) >= 8 else ImageOps.posterize(im, int(arg))
        elif op == 5:
            im = ImageOps.solarize(im, int(arg))
        elif op == 6:
            lut = [min(255, i + int(arg)) if i < 128 else i for i in range(256)]
            im = im.point(lut + lut + lut)
        elif op in (7, 8, 9, 10):
            im = (ImageEnhance.Color, ImageEnhance.Contrast, ImageEnhance.Brightness, ImageEnhance.Sharpness)[op - 7](im).enhance(arg)
        elif op in (11, 12, 13, 14):
            im = im.transform(im.size, Image.AFFINE, tuple(m), **kw)
    x = (np.asarray(im, dtype=np.float32).transpose(2, 0, 1) / 255.0 - mean) / std
    t, l, eh, ew = ebox
    if eh and ew:
        x[:, t:t + eh, l:l + ew] = rs.standard_normal((3, eh, ew)).astype(np.float32)
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("gpu", "pil"), required=True)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--stored", type=int, default=256)
    ap.add_argument("--bank", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--step-ms", type=float, default=33.6, help="the fine-tune step to set the figures beside")
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    from ssl4gie_amd.data import RANDAUG_OPS, MAEFinetuneTransform
    B, S, M = a.batch, a.size, a.stored
    rows = []

    def emit(r):
        r = {"part": a.part, **r}
        rows.append(r)
        print(json.dumps(r), flush=True)

    if a.part == "pil":
        from PIL import Image
        g = torch.Generator().manual_seed(0)
        tf = MAEFinetuneTransform(S, generator=g, noise_seed=0)
        n = min(B, 256)
        rs = np.random.RandomState(0)
        imgs = [Image.fromarray(rs.randint(0, 256, (M, M, 3)).astype(np.uint8), "RGB") for _ in range(8)]
        box, flip, layers, ebox, _ = tf.draw(n, M, M, "cpu")
        op, arg, matrix = (t.numpy() for t in layers)
        mean = np.array(tf.mean, np.float32).reshape(3, 1, 1)
        std = np.array(tf.std, np.float32).reshape(3, 1, 1)
        per = []
        for rep in range(3):
            t0 = time.perf_counter()
            for b in range(n):
                row = [(int(op[l, b]), float(arg[l, b]), matrix[l, b]) for l in range(op.shape[0])]
                pil_image(imgs[b % 8], S, box[b].tolist(), int(flip[b]), row, tf.randaug.fill, mean, std, ebox[b].tolist(), rs)
            per.append((time.perf_counter() - t0) / n * 1e3)
        emit({"what": "PIL path on a host CPU, one process: crop + bicubic resize + flip + 2 RandAugment layers + "
                      "ToTensor + Normalize + erase", "images": n, "stored": M, "size": S,
              "host_ms_per_image": round(statistics.median(per), 4), "min": round(min(per), 4), "max": round(max(per), 4),
              "host_ms_per_256_images_one_core": round(statistics.median(per) * 256, 1)})
    else:
        from ssl4gie_amd import _lib, ops
        from ssl4gie_amd.data import DeviceImageBank
        _lib.load()
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        g = torch.Generator(device=dev).manual_seed(0)
        bank = DeviceImageBank(torch.randint(0, 256, (a.bank, M, M, 3), dtype=torch.uint8, device=dev, generator=g))
        tf = MAEFinetuneTransform(S, generator=g, noise_seed=0)
        n_sets = a.warmup + a.reps
        sets = [tf.draw(B, M, M, dev) for _ in range(n_sets)]
        index = [torch.randint(0, a.bank, (B,), device=dev, generator=g) for _ in range(n_sets)]
        pix = float(B * S * S)
        emit({"batch": B, "size": S, "stored": M, "bank_images": a.bank, "warmup": a.warmup, "reps": a.reps,
              "device": torch.cuda.get_device_name(0), "config": "rand-m9-mstd0.5-inc1, re_prob 0.25, pixel"})

        def row(what, fn, floor_bytes=None, **extra):
            d, lo, hi = measure(fn, a.warmup, a.reps)
            r = {"what": what, "device_ms": round(d, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4),
                 "share_of_step": round(d / a.step_ms, 4)}
            if floor_bytes:
                r.update(floor_MB=round(floor_bytes / 1e6, 1), TB_per_s_of_floor_bytes=round(floor_bytes / (d * 1e-3) / 1e12, 3))
            r.update(extra)
            emit(r)
            return d

        crop = lambda it: ops.view_sample_u8(bank.images, index[it], sets[it][0], sets[it][1], S, "bicubic",
                                             tf.crop.mean, tf.crop.std)
        xs = [crop(i) for i in range(4)]
        u8 = [ops.quantize_u8(x) for x in xs]
        out = torch.empty_like(u8[0])
        ws = ops.randaug_layer_workspace(B, dev)
        layer = lambda it, l: ops.randaug_layer(u8[it % 4], sets[it][2][0][l], sets[it][2][1][l], sets[it][2][2][l],
                                                tf.randaug.fill, out, ws)
        row("a. drawing one batch's parameters (torch ops): crop, RandAugment, erase", lambda it: tf.draw(B, M, M, dev))
        row("b. view_sample_u8: crop + bicubic resample + flip", crop)
        row("c. quantize_u8", lambda it: ops.quantize_u8(xs[it % 4], out), 15.0 * pix)
        for l in range(tf.randaug.layers):
            row(f"d{l + 1}. randaug_layer, layer {l + 1} of the recipe's draws (half the samples skipped)",
                lambda it, l=l: layer(it, l), 6.0 * pix)
        mags = torch.full((B,), 9.0, dtype=torch.float64, device=dev)
        neg = torch.arange(B, device=dev) % 2 == 1
        from ssl4gie_amd.data import randaug_level_args
        for o, name in enumerate(RANDAUG_OPS):
            ids = torch.full((B,), o, dtype=torch.int64, device=dev)
            arg, matrix = randaug_level_args(ids, mags, neg, 1, S)
            op8 = ids.to(torch.uint8)
            row(f"d-{name}. randaug_layer, op {o} on every sample at magnitude 9",
                lambda it: ops.randaug_layer(u8[it % 4], op8, arg, matrix, tf.randaug.fill, out, ws),
                (9.0 if o in (0, 1, 8) else 6.0) * pix)
        row("e. normalize_erase_u8 on the recipe's boxes (pixel noise)",
            lambda it: ops.normalize_erase_u8(u8[it % 4], sets[it][3], "pixel", sets[it][4], tf.mean, tf.std), 15.0 * pix)
        row("f. MAEFinetuneTransform()(bank, index): a + b + c + d1 + d2 + e", lambda it: tf(bank, index[it]))
    if a.log:
        with open(a.log, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
