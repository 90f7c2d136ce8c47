#!/usr/bin/env python
"""Cost of the backward through fixed BatchNorm statistics (ssl4gie_bn_bwd_frozen) beside what the library offered
before it, per map and per ResNet50 step.

Maps: the bf16 BatchNorm maps of a ResNet50 step (the (stage, width) kinds bn_checks.PRODUCTION lists for 256 x 224²)
at the two batch geometries frozen statistics are used at: 4 x 1024² (detection) and 128 x 224².

Per map, device time (HIP events around the call, --warmup + --reps repetitions, median), in --passes passes whose
medians give the run-to-run spread; inside a pass the variants ALTERNATE repetition by repetition, so drift of the
machine hits all of them alike:
  frozen Y / BITS              the new entry point without parameter gradients (BITS writes dres, as it must)
  frozen Y / BITS + grads      ... with dgamma / dbeta: one reduction pass that also writes dx (and dres), + the tail
  parent Y / BITS              the closest formulation without it: ssl4gie_bn_bwd_apply with zero sums (BITS: the
                               reduce half for dres, then apply on it)
  parent Y / BITS + grads      ssl4gie_bn_bwd_reduce + ssl4gie_bn_bwd_apply with zero sums
  training Y / BITS            ssl4gie_bn_bwd (batch statistics: two passes)
Each as µs and as the share of its byte floor: the streams the formulation has to read and write, at --hbm-tbs
(DESIGN.md §5 uses 8 TB/s).  A map smaller than the 256 MiB Infinity Cache is partly served from it in a burst of
repeats: the shares of the small maps are upper bounds.
`verdict`: the frozen form without parameter gradients against its parent formulation — "slower" only when its median
exceeds the parent's by more than the parent's own spread over the passes.

Steps: one ResNet50 forward + backward (bf16) with norm_layer=FrozenBatchNorm2d after freeze_stages(5) against the
same trunk with nn.BatchNorm2d in training mode, at both geometries.

One JSON line per row; --log FILE appends them.

    timeout 600 python tools/time_frozen_bn.py --log profiles/frozen_bn_timing.log
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STAGES = ((2, 64), (4, 64), (4, 256), (4, 128), (8, 128), (8, 512), (8, 256), (16, 256), (16, 1024), (16, 512),
          (32, 512), (32, 2048))      # (stride of the map, channels) of the BatchNorm maps of torchvision's ResNet50


def maps_of(batch, size):
    return [(batch * (size // s) ** 2, C) for s, C in STAGES]


def alternate(fns, warmup, reps):
    """-> per fn the list of device times [ms]; repetition i of every fn before repetition i + 1 of any"""
    ms = [[] for _ in fns]
    for it in range(warmup + reps):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if it >= warmup:
                ms[k].append(e0.elapsed_time(e1))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--hbm-tbs", type=float, default=8.0)
    ap.add_argument("--step-reps", type=int, default=5)
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    from ssl4gie_amd import _lib, ops
    _lib.load()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rows_out = []

    def emit(r):
        rows_out.append(r)
        print(json.dumps(r), flush=True)

    emit({"device": torch.cuda.get_device_name(0), "warmup": a.warmup, "reps": a.reps, "passes": a.passes,
          "hbm_TB_per_s": a.hbm_tbs, "dtype": "bf16"})
    Y, BITS, NONE = _lib.BN_MASK_Y, _lib.BN_MASK_BITS, _lib.BN_MASK_NONE
    g = torch.Generator(device=dev).manual_seed(0)
    for geometry, (batch, size) in (("4x1024", (4, 1024)), ("128x224", (128, 224))):
        for rows, C in maps_of(batch, size):
            rn = lambda *s: torch.randn(*s, generator=g, device=dev)
            x = rn(rows, C).to(torch.bfloat16)
            dy = rn(rows, C).to(torch.bfloat16)
            gamma, beta, mean = rn(C), 0.3 * rn(C), 0.1 * rn(C)
            rstd = torch.rsqrt(0.5 + torch.rand(C, generator=g, device=dev))
            y, bits = ops.bn_apply_bits(x, ops.bn_coef_stats(mean, rstd, gamma, beta), None)
            zeros = torch.zeros(2, C, device=dev)
            dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)

            def parent_bits(grads):
                _, dres = ops.bn_bwd_reduce_bits(dy, bits, x, mean, rstd)
                return ops.bn_bwd_apply(dres, None, x, gamma, mean, rstd, zeros, 1.0, False)

            def parent_y_grads():
                ops.bn_bwd_reduce(dy, y, x, mean, rstd, True, False)
                return ops.bn_bwd_apply(dy, y, x, gamma, mean, rstd, zeros, 1.0, True)
            # (name, call, streams of rows x C x 2 bytes it has to move)
            variants = [
                ("frozen Y", lambda: ops.bn_bwd_frozen(dy, Y, y, None, gamma, None, None, rstd, False, None, None, False), 3),
                ("parent Y", lambda: ops.bn_bwd_apply(dy, y, x, gamma, mean, rstd, zeros, 1.0, True), 4),
                ("frozen BITS", lambda: ops.bn_bwd_frozen(dy, BITS, bits, None, gamma, None, None, rstd, True, None, None, False), 3.0625),
                ("parent BITS", lambda: parent_bits(False), 6.0625),
                ("frozen Y + grads", lambda: ops.bn_bwd_frozen(dy, Y, y, x, gamma, None, mean, rstd, False, dg, db, False), 4),
                ("parent Y + grads", parent_y_grads, 7),
                ("frozen BITS + grads", lambda: ops.bn_bwd_frozen(dy, BITS, bits, x, gamma, None, mean, rstd, True, dg, db, False), 4.0625),
                ("parent BITS + grads", lambda: parent_bits(True), 6.0625),
                ("training Y", lambda: ops.bn_bwd(dy, y, x, gamma, mean, rstd, True, False, dg, db, False), 7),
                ("training BITS", lambda: ops.bn_bwd_bits(dy, bits, x, gamma, mean, rstd, dg, db, False), 6.0625),
            ]
            med = {name: [] for name, _, _ in variants}
            for _ in range(a.passes):
                for (name, _, _), ms in zip(variants, alternate([fn for _, fn, _ in variants], a.warmup, a.reps)):
                    med[name].append(statistics.median(ms))
            mb = rows * C * 2 / 1e6
            out = {"geometry": geometry, "rows": rows, "C": C, "map_MB": round(mb, 2)}
            for name, _, streams in variants:
                us = statistics.median(med[name]) * 1e3
                floor_us = streams * mb / a.hbm_tbs     # MB / (TB/s) = µs
                out[name] = {"us": round(us, 2), "spread_us": round((max(med[name]) - min(med[name])) * 1e3, 2),
                             "streams": streams, "share_of_floor": round(floor_us / us, 3)}
            for kind in ("Y", "BITS", "Y + grads", "BITS + grads"):
                new, old = out["frozen " + kind], out["parent " + kind]
                out["ratio " + kind] = round(new["us"] / old["us"], 3)
                out["verdict " + kind] = "slower" if new["us"] > old["us"] + old["spread_us"] else "not slower"
            emit(out)
            del x, dy, y, bits
    if not a.skip_steps:
        from ssl4gie_amd.Models.resnet import FrozenBatchNorm2d, ResNet50
        for geometry, (batch, size) in (("4x1024", (4, 1024)), ("128x224", (128, 224))):
            imgs = torch.randn(batch, 3, size, size, generator=g, device=dev)
            out = {"step": "ResNet50 forward + backward, bf16", "geometry": geometry}
            models = {}
            for name in ("frozen", "training"):
                torch.manual_seed(0)
                m = ResNet50(norm_layer=FrozenBatchNorm2d if name == "frozen" else None).to(dev)
                m.set_precision("bf16")
                if name == "frozen":
                    m.freeze_stages(5)
                models[name] = m.train()

            def step(m):     # gradients accumulate in the arena from the second step on, as in a driver without zero_grad
                m.forward_maps(imgs).float().mean().backward()
            ms = alternate([lambda: step(models["frozen"]), lambda: step(models["training"])], 3, a.step_reps)
            for name, t in zip(("frozen", "training"), ms):
                out[name + "_ms"] = round(statistics.median(t), 3)
                out[name + "_min_max_ms"] = [round(min(t), 3), round(max(t), 3)]
            out["ratio"] = round(out["frozen_ms"] / out["training_ms"], 3)
            emit(out)
            del models, imgs
            torch.cuda.empty_cache()
    if a.log:
        with open(a.log, "a") as f:
            for r in rows_out:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
