#!/usr/bin/env python
"""Cost of DeepLabV3+ on the engine (ssl4gie_amd/Models/deeplab.py on csrc/atrous_ops.hip) at the reference's size
(224 x 224, bf16): the training step (forward + backward + ArenaAdamW) at batch 16 (the reference's default) and 128, and
each new kernel alone beside torch's own device op of the same formulation on the same values (F.conv2d dilated /
grouped on channels_last tensors, F.interpolate), with the bytes each kernel has to move (its floor) and the rate that
makes of its time.

Device time by HIP events around `inner` back-to-back calls (a timed window is milliseconds), divided by `inner`;
medians over --reps windows, wall time beside it; every shape is warmed up first.  The kernel is timed before AND after
the torch op (`device_us`, `device_us_again`): the spread between the two is the noise of the box.  One JSON line per
row; --log FILE appends the rows gathered.  Nothing is caught: the first exception (a HIP error among them) ends the
process with a non-zero status after the rows gathered so far are written, and nothing more is started on the device:

    timeout -k 10 600 python tools/experiments/deeplab_bench.py --log profiles/deeplab_timing.log
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def measure(fn, warmup, reps, inner=1):
    """(median device ms by events, median wall ms) of one fn(); a window holds `inner` calls"""
    ms, wall = [], []
    for it in range(warmup + reps):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 128])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step-reps", type=int, default=10)
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
    from ssl4gie_amd.atrous_engine import DilatedConv3x3Fn
    from ssl4gie_amd.engine import GradSink, LPCache
    from ssl4gie_amd.losses import SoftDiceLoss
    from ssl4gie_amd.Models.deeplab import DeepLabV3Plus
    from ssl4gie_amd.optim import ArenaAdamW
    _lib.load()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    bf = torch.bfloat16
    S = a.size

    def emit(r):
        rows.append(r)
        print(json.dumps(r), flush=True)

    def kernel_row(name, ours, theirs, floor_bytes, inner=20):
        d0, w0 = measure(ours, a.warmup, a.reps, inner)
        dt, _ = measure(theirs, a.warmup, a.reps, inner)
        d1, _ = measure(ours, 1, a.reps, inner)
        emit({"kernel": name, "device_us": round(d0 * 1e3, 2), "device_us_again": round(d1 * 1e3, 2),
              "wall_us": round(w0 * 1e3, 2), "torch_device_us": round(dt * 1e3, 2), "floor_MB": round(floor_bytes / 1e6, 3),
              "TB_per_s_of_floor": round(floor_bytes / (max(d0, d1) * 1e-3) / 1e12, 3),
              "torch_over_device": round(dt / max(d0, d1), 2)})

    emit({"device": torch.cuda.get_device_name(0), "size": S, "precision": "bf16", "warmup": a.warmup, "reps": a.reps,
          "step_reps": a.step_reps})
    g = torch.Generator(device=dev).manual_seed(0)

    def rnd(*shape, dtype=bf):
        return torch.randn(*shape, device=dev, generator=g).to(dtype)

    def nchw(x):   # the same values as an NCHW-shaped channels_last tensor: torch's op on the same memory layout
        return x.permute(0, 3, 1, 2)

    for B in a.batches:
        h16, h4 = S // 16, S // 4
        # ---- dilated dense 3x3 (layer4: 512 -> 512 at 1/16, d = 2)
        x, w = rnd(B, h16, h16, 512), rnd(512, 512, 3, 3, dtype=torch.float32) / 64
        wl = w.to(bf).contiguous(memory_format=torch.channels_last)
        n = x.numel() * 2
        kernel_row(f"im2col3x3_dil B={B} {h16}x{h16}x512 d=2 (torch: the whole dilated F.conv2d)",
                   lambda: ops.im2col3x3_dil(x, 2), lambda: F.conv2d(nchw(x), wl, padding=2, dilation=2), 10 * n)
        sink, lp = GradSink(None), LPCache()
        kernel_row(f"dilated conv forward (patch matrix + GEMM) B={B} {h16}x{h16} 512->512 d=2",
                   lambda: DilatedConv3x3Fn.apply(x, w, 2, sink, lp), lambda: F.conv2d(nchw(x), wl, padding=2, dilation=2),
                   10 * n + 2 * n)
        # ---- depthwise 3x3: ASPP rate 12 at 1/16 (2048 ch) and block2 at 1/4 (304 ch)
        for (hh, C, d) in ((h16, 2048, 12), (h4, 304, 1)):
            x, dy, w = rnd(B, hh, hh, C), rnd(B, hh, hh, C), rnd(C, 1, 3, 3, dtype=torch.float32)
            wb = w.to(bf)
            n = x.numel() * 2
            kernel_row(f"dwconv3x3_fwd B={B} {hh}x{hh}x{C} d={d}", lambda: ops.dwconv3x3_fwd(x, w, d),
                       lambda: F.conv2d(nchw(x), wb, padding=d, dilation=d, groups=C), 2 * n)
            kernel_row(f"dwconv3x3_wgrad B={B} {hh}x{hh}x{C} d={d}", lambda: ops.dwconv3x3_wgrad(dy, x, d),
                       lambda: torch.nn.grad.conv2d_weight(nchw(x), wb.shape, nchw(dy), padding=d, dilation=d, groups=C),
                       2 * n)
        # ---- bilinear x4, align_corners=True: the decoder's 256-channel map and the fp32 logit map
        for (hh, C, dt) in ((h16, 256, bf), (h4, 1, torch.float32)):
            x, dy = rnd(B, hh, hh, C, dtype=dt), rnd(B, 4 * hh, 4 * hh, C, dtype=dt)
            es = x.element_size()
            xl = nchw(x).requires_grad_(True)
            kernel_row(f"bilinear_up_ac_fwd x4 B={B} {hh}x{hh}x{C} {str(dt)[6:]}", lambda: ops.bilinear_up_ac_fwd(x, 4),
                       lambda: F.interpolate(nchw(x), scale_factor=4, mode="bilinear", align_corners=True),
                       17 * x.numel() * es)
            yl = F.interpolate(xl, scale_factor=4, mode="bilinear", align_corners=True)
            kernel_row(f"bilinear_up_ac_bwd x4 B={B} {hh}x{hh}x{C} {str(dt)[6:]}", lambda: ops.bilinear_up_ac_bwd(dy, 4),
                       lambda: torch.autograd.grad(yl, xl, nchw(dy), retain_graph=True), 17 * x.numel() * es)

    # ---- the training step
    for B in a.batches:
        torch.manual_seed(0)
        m = DeepLabV3Plus("resnet50", encoder_weights=None, classes=1).to(dev).set_precision("bf16").train()
        opt = ArenaAdamW(m, list(m.parameters()), lr=1e-4)
        loss_fn = SoftDiceLoss()
        imgs = torch.randn(B, 3, S, S, device=dev, generator=g)
        tgt = (torch.rand(B, 1, S, S, device=dev, generator=g) > 0.5).float()

        def step():
            opt.zero_grad()
            loss_fn(m(imgs), tgt).backward()
            opt.step()

        def fwd():
            with torch.no_grad():
                m(imgs)

        d, w = measure(step, a.warmup, a.step_reps)
        df, _ = measure(fwd, 1, a.step_reps)
        h16, h4 = S // 16, S // 4
        # floors of the new kernels in one step (bf16 = 2 B): forward + data gradient + weight gradient each move the same
        # bytes again — dilated patch matrices 3 convs x 3 passes x 10 maps, depthwise 3 passes x (read + write), x4 maps
        floor = 2.0 * B * (3 * 3 * 10 * h16 * h16 * 512 + 3 * 2 * (3 * h16 * h16 * 2048 + h16 * h16 * 256 + h4 * h4 * 304)
                           + 2 * 17 * h16 * h16 * 256) + 4.0 * B * 2 * 17 * h4 * h4
        emit({"step": "forward + backward + ArenaAdamW", "batch": B, "device_ms": round(d, 3), "wall_ms": round(w, 3),
              "images_per_s": round(B / (w * 1e-3), 1), "eval_forward_device_ms": round(df, 3),
              "new_kernels_floor_MB": round(floor / 1e6, 1), "floor_ms_at_4TB_per_s": round(floor / 4e12 * 1e3, 3)})
        del m, opt


if __name__ == "__main__":
    main()
