#!/usr/bin/env python
"""Cost of a linear-probe step on the engine and of the device code around its frozen trunk (ssl4gie_amd/probe.py):

  --part step    a. ViT-B/16 at batch 256 with bf16 operands on synthetic resident data, `probe.mae_linear_probe`:
                 the frozen forward alone (forward_features under no_grad), the head (BatchNorm + product +
                 CrossEntropyLoss + backward) on given features, the ranged LARS step, and the whole probe step;
                 beside them the fine-tune step of the same model (every parameter trainable, ArenaAdamW), the
                 variants ALTERNATING call by call in one process
  --part score   b. metrics.TopKAccuracy over a 40-batch loader (B = 256, C = 1000) with its one read-back, against the
                 drivers' formulation on the same device tensors: accuracy(output, target, topk=(1, 5)) by torch.topk
                 plus three .item() per batch (loss, acc1, acc5: main_lincls.py:365-368)
  --part optim   c. one ranged LARS step on the ViT-B head against optim.ArenaLARS over the whole arena (same
                 parameters, same gradients), with the bytes of optimizer state each keeps;
                 d. optim.ArenaSGD on ResNet50's fc against torch.optim.SGD on the same two parameters

Device time: HIP events around the call (the scoring loop: a host clock around work that ends in its read-back, since
the read-backs are the point), 10 warm-up + 30 timed repetitions per variant, medians (min, max).  One JSON line per
row; --log FILE appends them.  Run each part as a process of its own, under a time limit:

    timeout 300 python tools/time_linprobe.py --part step --log profiles/linprobe_timing.log
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def measure_alternating(fns, warmup, reps, host_clock=False):
    """{name: fn(it)} timed in rotation (a, b, a, b, ...) -> {name: (median, min, max)} in ms"""
    ms = {k: [] for k in fns}
    for it in range(warmup + reps):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            if host_clock:
                t0 = time.perf_counter()
                fn(it)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
            else:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn(it)
                e1.record()
                torch.cuda.synchronize()
                dt = e0.elapsed_time(e1)
            if it >= warmup:
                ms[name].append(dt)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}


def emit(row, log):
    line = json.dumps(row)
    print(line, flush=True)
    if log:
        with open(log, "a") as f:
            f.write(line + "\n")


def rows_of(part, res, names, log, **extra):
    for k, (med, lo, hi) in res.items():
        emit({"part": part, "what": names[k], "ms": round(med, 4), "min": round(lo, 4), "max": round(hi, 4),
              **extra.get(k, {})}, log)


def part_step(args):
    from ssl4gie_amd.losses import CrossEntropyLoss
    from ssl4gie_amd.Models.mae import models_vit
    from ssl4gie_amd.Models.mae.util.lars import LARS
    from ssl4gie_amd.optim import ArenaAdamW
    from ssl4gie_amd.probe import mae_linear_probe
    B, dev = args.batch, "cuda"
    torch.manual_seed(0)
    probe = mae_linear_probe(models_vit.vit_base_patch16(num_classes=1000)).to(dev).set_precision("bf16").train()
    tuned = models_vit.vit_base_patch16(num_classes=1000).to(dev).set_precision("bf16").train()
    x = torch.randn(B, 3, 224, 224, device=dev)
    y = torch.randint(0, 1000, (B,), device=dev)
    crit = CrossEntropyLoss()
    lars = LARS(probe.head.parameters(), lr=0.1 * B / 256, weight_decay=0.0)
    adamw = ArenaAdamW(tuned, [p for p in tuned.parameters()], lr=1e-5)
    with torch.no_grad():
        feats = probe.forward_features(x)

    def trunk(it):
        with torch.no_grad():
            probe.forward_features(x)

    def head(it):
        lars.zero_grad()
        crit(probe.forward_head(feats), y).backward()

    def probe_step(it):
        loss = crit(probe(x), y)
        lars.zero_grad()
        loss.backward()
        lars.step()

    def tune_step(it):
        loss = crit(tuned(x), y)
        loss.backward()
        adamw.step()
        adamw.zero_grad()

    head(0)
    res = measure_alternating({"trunk": trunk, "head": head, "lars": lambda it: lars.step(), "probe": probe_step,
                               "tune": tune_step}, args.warmup, args.reps)
    n_head = sum(p.numel() for p in probe.head.parameters())
    names = {"trunk": f"ViT-B/16 frozen forward B={B} bf16 (forward_features, no_grad)",
             "head": f"probe head on given features: BatchNorm + [{B}, 768] x [768, 1000] + CrossEntropyLoss + backward",
             "lars": f"ranged LARS step over the head ({n_head} elements)",
             "probe": f"ViT-B/16 probe step B={B} bf16: frozen forward + head + LARS",
             "tune": f"ViT-B/16 fine-tune step B={B} bf16: forward + CrossEntropyLoss + backward + ArenaAdamW"}
    rows_of("a", res, names, args.log)
    emit({"part": "a", "what": "head + LARS share of the probe step",
          "share": round((res["head"][0] + res["lars"][0]) / res["probe"][0], 4)}, args.log)


def part_score(args):
    from ssl4gie_amd.metrics import TopKAccuracy
    B, C, nb, dev = args.batch, 1000, 40, "cuda"
    g = torch.Generator(dev).manual_seed(0)
    logits = [torch.randn(B, C, device=dev, generator=g) for _ in range(nb)]
    targets = [torch.randint(0, C, (B,), device=dev, generator=g) for _ in range(nb)]
    out = {}

    def fused(it):
        m = TopKAccuracy((1, 5))
        for lg, tg in zip(logits, targets):
            m.update(lg, tg)
        out["fused"] = m.compute()

    def drivers(it):
        n = top1 = top5 = loss = 0.0
        for lg, tg in zip(logits, targets):
            l = torch.nn.functional.cross_entropy(lg, tg)
            _, pred = lg.topk(5, 1, True, True)
            correct = pred.t().eq(tg.view(1, -1).expand_as(pred.t()))
            acc1 = correct[:1].reshape(-1).float().sum(0, keepdim=True).mul_(100.0 / B)
            acc5 = correct[:5].reshape(-1).float().sum(0, keepdim=True).mul_(100.0 / B)
            loss += l.item() * B
            top1 += acc1[0].item() * B
            top5 += acc5[0].item() * B
            n += B
        out["drivers"] = {"acc1": top1 / n, "acc5": top5 / n, "loss": loss / n}

    res = measure_alternating({"fused": fused, "drivers": drivers}, args.warmup, args.reps, host_clock=True)
    names = {"fused": f"TopKAccuracy over {nb} batches [{B}, {C}] fp32, one read-back (host clock)",
             "drivers": f"accuracy(topk=(1, 5)) + CrossEntropyLoss + 3 .item() per batch, {nb} batches (host clock)"}
    rows_of("b", res, names, args.log)
    emit({"part": "b", "what": "the two formulations' results", "fused": out["fused"], "drivers": out["drivers"]},
         args.log)


def part_optim(args):
    from ssl4gie_amd.Models.mae import models_vit
    from ssl4gie_amd.Models.mae.util.lars import LARS
    from ssl4gie_amd.Models.resnet import resnet50
    from ssl4gie_amd.optim import ArenaLARS, ArenaSGD
    from ssl4gie_amd.probe import mae_linear_probe, moco_linear_probe
    dev = "cuda"
    torch.manual_seed(0)
    m = mae_linear_probe(models_vit.vit_base_patch16(num_classes=1000)).to(dev).set_precision("bf16")
    a = m.arena()
    own = list(m.head.parameters())
    for p in own:
        p.grad = a.grad_view(p)
        p.grad.normal_()
    ranged = LARS(m.head.parameters(), lr=1e-3, weight_decay=0.0)
    whole = ArenaLARS(m, own, lr=1e-3, weight_decay=0.0)
    res = measure_alternating({"ranged": lambda it: ranged.step(), "whole": lambda it: whole.step()}, args.warmup,
                              args.reps)
    names = {"ranged": "ranged LARS step on the ViT-B head", "whole": "ArenaLARS step over the whole ViT-B arena"}
    rows_of("c", res, names, args.log, ranged={"state_MB": round(4e-6 * ranged.mu.numel(), 2)},
            whole={"state_MB": round(4e-6 * whole.mu.numel(), 2)})
    del m, ranged, whole

    r = moco_linear_probe(resnet50(num_classes=1000), "fc").to(dev).set_precision("bf16")
    ra = r.arena()
    fc = [r.fc.weight, r.fc.bias]
    for p in fc:
        p.grad = ra.grad_view(p)
        p.grad.normal_()
    sgd = ArenaSGD(r, fc, 0.1, momentum=0.9, weight_decay=0.0)
    twin = [torch.nn.Parameter(p.detach().clone()) for p in fc]
    for q, p in zip(twin, fc):
        q.grad = p.grad.detach().clone()
    tsgd = torch.optim.SGD(twin, 0.1, momentum=0.9, weight_decay=0.0)
    res = measure_alternating({"arena": lambda it: sgd.step(), "torch": lambda it: tsgd.step()}, args.warmup, args.reps)
    names = {"arena": "ArenaSGD step on ResNet50's fc (2048 x 1000 + 1000)", "torch": "torch.optim.SGD step on the same"}
    rows_of("d", res, names, args.log)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("step", "score", "optim"), required=True)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_linprobe.py measures on the MI355X: no GPU found (there is no CPU fallback)")
    torch.cuda.set_device(0)
    {"step": part_step, "score": part_score, "optim": part_optim}[args.part](args)


if __name__ == "__main__":
    main()
