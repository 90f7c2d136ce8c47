#!/usr/bin/env python
"""Cost of the on-device finetune augmentation (ssl4gie_amd.data.FinetuneAugment.segmentation: ops.normalize_u8 ->
ops.color_augment_ft -> ops.paired_warp) at B = 128, S = 224, split into its steps, beside the same recipe's blur and
warp written in torch ops on the device, and the 32-row against the 16-row tile of the 25-tap colour kernel.

  --part fused   a. parameter draw (torch ops); b. gather + normalize_u8; c. color_augment_ft on the recipe's draws;
                 d. paired_warp, image + uint8 mask; e. the whole transform call; c2. the colour stage with one sigma
                 on every sample, radius by radius
  --part torch   the baseline to beat, same parameters: the 25-tap blur as reflect F.pad + one grouped F.conv2d pair
                 (per-sample kernels, horizontal then vertical), and the flips + affine as torch.flip / torch.where,
                 torchvision's base grid, bmm and F.grid_sample(nearest) on image and mask.  The jitter has no
                 compact torch-op form and is left out of the baseline: compare its rows with c. minus the jitter-only
                 time (c0.) and with d.
  --part ab --ab-lib LIB   color_augment_ft of the package's library (CA_FT_TILE_H as built) against the same entry
                 point of LIB, a library of color_ops.hip alone built with the other tile height:
                     hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=fast -Issl4gie_amd/csrc -Iinclude \\
                         -DCA_FT_TILE_H=16 -shared ssl4gie_amd/csrc/color_ops.hip -o color_ops_ft16.so

Byte floor: the colour stage reads and writes the fp32 image once each, 24 B per pixel (the statistics pass reads it
once more: 36); the warp reads and writes image (24 B) and mask (1 + 4 B), 29 B per pixel.  Device time: HIP events
around the call, inputs in rotation over a pool larger than the Infinity Cache, 10 warm-up + 50 timed repetitions,
medians.  One JSON line per row; --log FILE appends them.  Run each part as a process of its own, under a time limit:

    timeout 300 python tools/time_finetune_augment.py --part fused --log profiles/finetune_augment_timing.log
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

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


def torch_blur(x, sigma):
    """transforms.GaussianBlur((25, 25)) with one sigma per sample: reflect pad + depthwise conv2d, as two 1-D passes"""
    B, _, S, _ = x.shape
    k = torch.arange(-12, 13, device=x.device, dtype=torch.float32).view(1, 25)
    w = torch.exp(-0.5 * (k / sigma.clamp_min(1e-6).view(B, 1)) ** 2)
    w = (w / w.sum(dim=1, keepdim=True)).repeat_interleave(3, dim=0)                     # [3 B, 25]
    y = F.pad(x, (12, 12, 12, 12), mode="reflect").view(1, 3 * B, S + 24, S + 24)
    y = F.conv2d(y, w.view(3 * B, 1, 1, 25), groups=3 * B)
    return F.conv2d(y, w.view(3 * B, 1, 25, 1), groups=3 * B).view(B, 3, S, S)


def torch_warp(x, mask, matrix, flip, fill):
    """TF.hflip / TF.vflip where the bits say so, then TF.affine's tensor path on image and mask"""
    B, _, S, _ = x.shape
    both = torch.cat([x, mask, torch.ones_like(mask)], dim=1)
    h, v = (flip & 1).view(B, 1, 1, 1) != 0, (flip & 2).view(B, 1, 1, 1) != 0
    both = torch.where(h, both.flip(-1), both)
    both = torch.where(v, both.flip(-2), both)
    lin = torch.linspace(-S * 0.5 + 0.5, S * 0.5 - 0.5, S, device=x.device)
    base = torch.stack([lin.view(1, S).expand(S, S), lin.view(S, 1).expand(S, S), torch.ones(S, S, device=x.device)], dim=2)
    grid = base.view(1, S * S, 3).expand(B, -1, -1).bmm(matrix.view(B, 2, 3).transpose(1, 2) / (0.5 * S)).view(B, S, S, 2)
    out = F.grid_sample(both, grid, mode="nearest", padding_mode="zeros", align_corners=False)
    inside = out[:, 4:5] >= 0.5
    return torch.where(inside, out[:, :3], fill.view(1, 3, 1, 1)), torch.where(inside, out[:, 3:4], 0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("fused", "torch", "ab"), required=True)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--bank", type=int, default=4096, help="images in the bank (2.4 GB of fp32 batches pass through per 50 reps)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--ab-lib", default=None)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()

    from ssl4gie_amd import _lib, ops
    from ssl4gie_amd.data import DeviceImageBank, FinetuneAugment
    L = _lib.load()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, S, n = a.batch, a.size, a.bank
    rows = []

    def emit(r):
        r = {"part": a.part, **r}
        rows.append(r)
        print(json.dumps(r), flush=True)

    g = torch.Generator(device=dev).manual_seed(0)
    bank = DeviceImageBank(torch.randint(0, 256, (n, S, S, 3), dtype=torch.uint8, device=dev, generator=g),
                           targets=torch.randint(0, 256, (n, S, S), dtype=torch.uint8, device=dev, generator=g))
    tf = FinetuneAugment.segmentation(S, generator=g)
    n_sets = a.warmup + a.reps
    sets = [tf.draw(B, dev) for _ in range(n_sets)]
    index = [torch.randint(0, n, (B,), device=dev, generator=g) for _ in range(n_sets)]
    pool = [ops.normalize_u8(bank.images[index[i]], (0.0,) * 3, (1.0,) * 3) for i in range(16)]   # 16 x 77 MB
    pix = float(B * S * S)
    emit({"batch": B, "size": S, "bank_images": n, "warmup": a.warmup, "reps": a.reps,
          "device": torch.cuda.get_device_name(0), "tile_rows_as_built": "CA_FT_TILE_H of the library"})

    def row(what, fn, floor_bytes=None, **extra):
        d, lo, hi = measure(fn, a.warmup, a.reps)
        r = {"what": what, "device_ms": round(d, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4)}
        if floor_bytes:
            r.update(floor_MB=round(floor_bytes / 1e6, 1), TB_per_s_of_floor_bytes=round(floor_bytes / (d * 1e-3) / 1e12, 3))
        r.update(extra)
        emit(r)
        return d

    out = torch.empty_like(pool[0])
    color = lambda it, sigma=None: ops.color_augment_ft(pool[it % 16], *sets[it][:3], sets[it][3] if sigma is None else sigma,
                                                        tf.mean, tf.std, out=out)
    if a.part == "fused":
        row("a. drawing one batch's parameters (torch ops)", lambda it: tf.draw(B, dev))
        row("b. gather of the batch's uint8 rows + normalize_u8", lambda it: ops.normalize_u8(bank.images[index[it]], (0.0,) * 3, (1.0,) * 3),
            15.0 * pix + 6.0 * pix)
        zero = torch.zeros(B, device=dev)
        row("c0. color_augment_ft, jitter alone (sigma = 0 on every sample)", lambda it: color(it, zero), 36.0 * pix)
        row("c. color_augment_ft, segmentation recipe (sigma in [0.001, 2])", color, 36.0 * pix)
        for s in (0.3, 0.6, 1.0, 1.3, 1.6, 2.0):
            fixed = torch.full((B,), s, device=dev)
            row(f"c2. color_augment_ft, sigma = {s} on every sample", lambda it: color(it, fixed), 36.0 * pix)
        row("d. paired_warp, image + uint8 mask", lambda it: ops.paired_warp(pool[it % 16], sets[it][5], sets[it][4], tf.fill,
                                                                            bank.targets, index[it], 0.0), 29.0 * pix)
        row("e. FinetuneAugment.segmentation()(bank, index): a + b + c + d", lambda it: tf(bank, index[it]))
    elif a.part == "torch":
        fill = torch.tensor(tf.fill, device=dev)
        masks = [bank.targets[index[i]].unsqueeze(1).to(torch.float32) / 255.0 for i in range(16)]
        row("t1. torch ops: reflect pad + two grouped conv2d passes, per-sample sigma", lambda it: torch_blur(pool[it % 16], sets[it][3]))
        row("t2. torch ops: flips + base grid + bmm + grid_sample(nearest) on image and mask",
            lambda it: torch_warp(pool[it % 16], masks[it % 16], sets[it][5], sets[it][4], fill))
        row("t1 + t2", lambda it: torch_warp(torch_blur(pool[it % 16], sets[it][3]), masks[it % 16], sets[it][5], sets[it][4], fill))
    else:
        if not a.ab_lib:
            raise SystemExit("--part ab needs --ab-lib")
        other = C.CDLL(os.path.abspath(a.ab_lib))
        other.ssl4gie_color_augment_ft.restype = C.c_int
        other.ssl4gie_color_augment_ft.argtypes = _lib.PROTOTYPES["ssl4gie_color_augment_ft"][1]
        ws = torch.empty(L.ssl4gie_color_augment_workspace_bytes(B, S), dtype=torch.uint8, device=dev)
        m, s = (C.c_float * 3)(*tf.mean), (C.c_float * 3)(*tf.std)

        def direct(lib):
            def fn(it, sigma=None):
                f, o, fl, sg = sets[it][:4]
                sg = sg if sigma is None else sigma
                rc = lib.ssl4gie_color_augment_ft(pool[it % 16].data_ptr(), out.data_ptr(), B, S, f.data_ptr(), o.data_ptr(), fl.data_ptr(),
                                                  sg.data_ptr(), m, s, ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
                assert rc == 0, rc
            return fn

        direct(L)(0)
        ref = out.clone()
        direct(other)(0)
        emit({"what": "the two libraries give the same bits on one batch", "equal": bool(torch.equal(ref, out))})
        two = torch.full((B,), 2.0, device=dev)
        for name, lib in (("package library", L), (os.path.basename(a.ab_lib), other)):
            fn = direct(lib)
            row(f"color_augment_ft, segmentation recipe: {name}", fn, 36.0 * pix)
            row(f"color_augment_ft, sigma = 2 on every sample: {name}", lambda it: fn(it, two), 36.0 * pix)
    if a.log:
        with open(a.log, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
