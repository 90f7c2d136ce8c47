#!/usr/bin/env python
"""Cost of the MAE fine-tuning recipe on the engine (Models/mae/models_vit.py, data.Mixup, the soft-target losses):
ViT-B/16 at batch 256 with bf16 operands on synthetic resident data — forward, SoftTargetCrossEntropy, backward and
ArenaAdamW over the 28 layer-decay groups of util/lr_decay.param_groups_lrd.

  --part step    a. the whole step with drop_path_rate = 0 against 0.1 (the same model, the blocks' rates switched;
                 the two variants ALTERNATE step by step in one process);
                 a2. the two stochastic-depth kernels alone on the step's [256 x 197, 768] fp32 stream, with the
                 bytes they move: ssl4gie_drop_path_add reads res and t and writes out (12 B / element, 8 B for a
                 dropped sample), ssl4gie_drop_path_scale_cast reads dx and writes the bf16 copy (6 B / element)
  --part mixup   b. data.Mixup's kernel pair against its torch formulation (data.mixup_torch + copy back,
                 data.mixup_target_torch) on the same device tensors, alternated; tables: blend only, box only, and a
                 per-sample mixture.  Byte floor of the image kernel: one read and one write of the batch
  --part loss    c. SoftTargetCrossEntropy / LabelSmoothingCrossEntropy value and gradient at [256, 1000], the fused
                 kernels against the torch formulation (SSL4GIE_FUSED_LOSS=0), alternated

Device time: HIP events around the call, 10 warm-up + 30 timed repetitions per variant, medians (min, max).  One JSON
line per row; --log FILE appends them.  Run each part as a process of its own, under a time limit:

    timeout 300 python tools/time_finetune.py --part step --log profiles/finetune_recipe_timing.log
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def measure_alternating(fns, warmup, reps):
    """{name: fn(it)} timed in rotation (a, b, a, b, ...) -> {name: (median, min, max)} in ms"""
    ms = {k: [] for k in fns}
    for it in range(warmup + reps):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(it)
            e1.record()
            torch.cuda.synchronize()
            if it >= warmup:
                ms[name].append(e0.elapsed_time(e1))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}


def emit(rows, row, log):
    line = json.dumps(row)
    print(line, flush=True)
    rows.append(line)
    if log:
        with open(log, "a") as f:
            f.write(line + "\n")


def part_step(args, rows):
    from ssl4gie_amd import _lib, ops
    from ssl4gie_amd.losses import SoftTargetCrossEntropy
    from ssl4gie_amd.Models.mae import models_vit
    from ssl4gie_amd.Models.mae.util.lr_decay import param_groups_lrd
    from ssl4gie_amd.optim import ArenaAdamW
    B, dev = args.batch, "cuda"
    torch.manual_seed(0)
    m = models_vit.vit_base_patch16(global_pool=True, num_classes=1000, drop_path_rate=0.1).to(dev).set_precision("bf16")
    m.train()
    rates = [b.drop_path for b in m.blocks]
    groups = param_groups_lrd(m, 0.05, no_weight_decay_list=m.no_weight_decay(), layer_decay=0.75)
    for g in groups:
        g["lr"] = 1e-4 * g["lr_scale"]
    opt = ArenaAdamW(m, groups, lr=1e-4, betas=(0.9, 0.999))
    x = torch.randn(B, 3, 224, 224, device=dev)
    t = torch.softmax(torch.randn(B, 1000, device=dev), dim=1)
    crit = SoftTargetCrossEntropy()

    def step(rate_on):
        for b, r in zip(m.blocks, rates):
            b.drop_path = r if rate_on else 0.0
        loss = crit(m(x), t)
        loss.backward()
        opt.step()
        opt.zero_grad()

    res = measure_alternating({"rate0": lambda it: step(False), "rate0.1": lambda it: step(True)}, args.warmup, args.reps)
    for k, (med, lo, hi) in res.items():
        emit(rows, {"part": "a", "what": f"ViT-B/16 step B={B} bf16, drop_path_rate {k[4:]}", "ms": round(med, 3),
                    "min": round(lo, 3), "max": round(hi, 3), "groups": len(groups)}, args.log)
    emit(rows, {"part": "a", "what": "stochastic depth, added ms per step",
                "ms": round(res["rate0.1"][0] - res["rate0"][0], 3)}, args.log)

    # a2. the two kernels alone
    L = _lib.load()
    T, D = B * 197, 768
    n = T * D
    bufs = [torch.randn(n, device=dev) for _ in range(3)]
    out = torch.empty(n, device=dev)
    out_lp = torch.empty(n, dtype=torch.bfloat16, device=dev)
    for share in (1.0, 0.9):
        s = (torch.rand(B, device=dev) < share).float() / share
        kept = float((s != 0).float().mean())

        def add(it):
            _lib.check(L.ssl4gie_drop_path_add(bufs[it % 3].data_ptr(), bufs[(it + 1) % 3].data_ptr(), s.data_ptr(),
                                               out.data_ptr(), B, 197 * D, ops.stream()), "drop_path_add")

        def cast(it):
            _lib.check(L.ssl4gie_drop_path_scale_cast(bufs[it % 3].data_ptr(), s.data_ptr(), out_lp.data_ptr(),
                                                      _lib.BF16, B, 197 * D, ops.stream()), "drop_path_scale_cast")

        res = measure_alternating({"add": add, "cast": cast}, args.warmup, args.reps)
        for k, nbytes in (("add", n * (8 + 4 * kept)), ("cast", n * (2 + 4 * kept))):
            med, lo, hi = res[k]
            emit(rows, {"part": "a2", "what": f"ssl4gie_drop_path_{'add' if k == 'add' else 'scale_cast (bf16)'} "
                        f"[{T}, {D}], kept share {kept:.3f}", "ms": round(med, 4), "min": round(lo, 4),
                        "max": round(hi, 4), "MB": round(nbytes / 1e6, 1), "TB/s": round(nbytes / med / 1e9, 2)}, args.log)


def part_mixup(args, rows):
    from ssl4gie_amd import data, ops
    B, dev = args.batch, "cuda"
    x0 = torch.randn(B, 3, 224, 224, device=dev)
    xs = [x0.clone() for _ in range(3)]   # 154 MB each: in rotation
    y = torch.randint(0, 1000, (B,), device=dev)
    nbytes = 2 * x0.numel() * 4
    for tag, kw in (("blend only", dict(mixup_alpha=0.8, cutmix_alpha=0.0)), ("box only", dict(mixup_alpha=0.0, cutmix_alpha=1.0)),
                    ("mixture", dict(mixup_alpha=0.8, cutmix_alpha=1.0))):
        lam, box, use = data.mixup_tables(np.random.RandomState(1), B, 224, 224, mode="elem", **kw)
        lam, box, use = (torch.from_numpy(a).to(dev) for a in (lam, box, use))

        def fused(it):
            ops.mixup(xs[it % 3], lam, box, use)
            ops.mixup_target(y, lam, 1000, 0.1)

        def torch_form(it):
            xi = xs[it % 3]
            xi.copy_(data.mixup_torch(xi, lam, box, use))
            data.mixup_target_torch(y, lam, 1000, 0.1)

        res = measure_alternating({"kernels": fused, "torch": torch_form}, args.warmup, args.reps)
        for k, (med, lo, hi) in res.items():
            emit(rows, {"part": "b", "what": f"Mixup elem B={B} 3x224x224, {tag}: {k}", "ms": round(med, 4),
                        "min": round(lo, 4), "max": round(hi, 4), "MB": round(nbytes / 1e6, 1),
                        "TB/s": round(nbytes / med / 1e9, 2)}, args.log)


def part_loss(args, rows):
    from ssl4gie_amd.losses import LabelSmoothingCrossEntropy, SoftTargetCrossEntropy
    B, Cn, dev = args.batch, 1000, "cuda"
    x = torch.randn(B, Cn, device=dev)
    t = torch.softmax(torch.randn(B, Cn, device=dev), dim=1)
    y = torch.randint(0, Cn, (B,), device=dev)
    for mod, arg in ((SoftTargetCrossEntropy(), t), (LabelSmoothingCrossEntropy(0.1), y)):
        def run(fused):
            os.environ["SSL4GIE_FUSED_LOSS"] = "1" if fused else "0"
            xr = x.clone().requires_grad_(True)
            mod(xr, arg).backward()

        res = measure_alternating({"kernels": lambda it: run(True), "torch": lambda it: run(False)}, args.warmup, args.reps)
        os.environ.pop("SSL4GIE_FUSED_LOSS", None)
        for k, (med, lo, hi) in res.items():
            emit(rows, {"part": "c", "what": f"{type(mod).__name__} [{B}, {Cn}] value + gradient: {k}",
                        "ms": round(med, 4), "min": round(lo, 4), "max": round(hi, 4)}, args.log)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["step", "mixup", "loss"], required=True)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the HIP device"
    rows = []
    {"step": part_step, "mixup": part_mixup, "loss": part_loss}[args.part](args, rows)


if __name__ == "__main__":
    main()
