#!/usr/bin/env python
"""Cost of the gradient norm / clip / scaler update on the MAE ViT-B model (B = 256, after one real backward):

  norm only   1. the reference expression  misc.get_grad_norm_(model.parameters())   (Models/mae/util/misc.py:280-292)
              2. torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm)        (max_norm huge: coefficient 1)
              3. the arena norm kernel      ssl4gie_amd.optim.get_grad_norm_(model)
              3b. optim.clip_grad_norm_(model, max_norm) with the clip live (norm pass + in-place scale pass)
              3k. the two kernels of 3 alone, 20 launches back to back over the same arena (part of each
                  repeat may come from the 256 MiB Infinity Cache)
              3h. the same burst alternating between the arena and a copy of it (2 x 448 MB in turn: nothing
                  a launch reads can still sit in the cache) -- the HBM bytes/s figure
  update      the whole `loss_scaler(loss, optimizer, ..., update_grad=True)` of engine_pretrain.py:55-57 with the
              backward pass excluded (the loss handed in is a detached leaf: its backward touches no parameter; the
              gradients of the one real backward stay in place), ArenaAdamW as the optimizer:
              torch-op scaler (GradScaler + per-tensor norms, as tests/test_gpu_reference_loop.py restates it)
              against ssl4gie_amd.Models.mae.util.misc.NativeScalerWithGradNormCount, without and with clip_grad.
              The torch-op scaler's unscale_ divides the gradients by the scale on every call; they are multiplied
              back outside the timed region.

Device time: HIP events around the call; host time: wall clock from the call to its return (no synchronisation
inside).  10 warm-up + 50 timed repetitions, medians.  One JSON line per row; --log FILE appends them to a file.

    python tools/time_grad_norm.py --log profiles/grad_norm_timing.log
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def param_groups(model, wd=0.05):
    decay, no_decay = [], []
    for n, p in model.named_parameters():
        if p.requires_grad:
            (no_decay if (p.ndim <= 1 or n.endswith(".bias")) else decay).append(p)
    return [{"params": no_decay, "weight_decay": 0.0}, {"params": decay, "weight_decay": wd}]


def measure(fn, warmup, reps, before=None):
    dev_ms, host_ms = [], []
    for it in range(warmup + reps):
        if before is not None:
            before()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        fn()
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
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--log", default=None)
    a = ap.parse_args()

    from ssl4gie_amd import _lib, optim
    from ssl4gie_amd.Models.mae import models_mae
    from ssl4gie_amd.Models.mae.util import misc
    _lib.load()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(0)
    model = models_mae.mae_vit_base_patch16(norm_pix_loss=True).to(dev).set_precision(a.precision)
    imgs = torch.randn(a.batch, 3, 224, 224, generator=torch.Generator("cpu").manual_seed(0)).to(dev)
    loss, _, _ = model(imgs, mask_ratio=0.75)
    loss.backward()
    torch.cuda.synchronize()
    arena = model.arena()
    params = list(model.parameters())
    n3 = optim.get_grad_norm_(model)   # (adopts any gradient that autograd left outside the arena)
    grads = [p.grad for p in params if p.grad is not None]
    nbytes = 4 * arena.numel
    rows = []

    def emit(r):
        rows.append(r)
        print(json.dumps(r), flush=True)

    def row(name, dev_ms, host_ms, **extra):
        emit({"what": name, "device_ms": round(dev_ms, 4), "host_ms": round(host_ms, 4), **extra})

    emit({"model": "mae_vit_base_patch16", "batch": a.batch, "precision": a.precision,
          "tensors_with_grad": len(grads), "arena_elements": arena.numel, "arena_MB": round(nbytes / 1e6, 1),
          "warmup": a.warmup, "reps": a.reps, "device": torch.cuda.get_device_name(0)})

    # ---- the norm alone
    ref64 = torch.cat([g.double().flatten() for g in grads]).norm().item()
    n1 = misc._torch_grad_norm(params, 2.0)
    emit({"fp64_norm": ref64, "rel_err_reference_fp32": abs(float(n1) - ref64) / ref64,
          "rel_err_arena_kernel": abs(float(n3) - ref64) / ref64})
    d, h = measure(lambda: misc._torch_grad_norm(params, 2.0), a.warmup, a.reps)
    row("1 reference get_grad_norm_ (torch ops)", d, h)
    d, h = measure(lambda: torch.nn.utils.clip_grad_norm_(params, 1e9), a.warmup, a.reps)
    row("2 torch.nn.utils.clip_grad_norm_", d, h)
    d, h = measure(lambda: optim.get_grad_norm_(model), a.warmup, a.reps)
    row("3 arena norm kernel (optim.get_grad_norm_)", d, h, TB_per_s=round(nbytes / (d * 1e-3) / 1e12, 3),
        fraction_of_8TBps=round(nbytes / (d * 1e-3) / 8e12, 3))
    # the kernels alone: 20 launches back to back between the events, so that the host's enqueue time (which the
    # single calls above are bound by) does not sit between them
    st = arena._grad_norm_state
    start, mask = st["dev"]

    def burst():
        for _ in range(20):
            st["gn"].run(arena, start, mask, len(arena.params))
    d, h = measure(burst, 3, 10)
    row("3k arena norm kernels alone (stage 1 + stage 2), per launch pair of a 20-launch burst", d / 20, h / 20,
        TB_per_s=round(nbytes / (d / 20 * 1e-3) / 1e12, 3), fraction_of_8TBps=round(nbytes / (d / 20 * 1e-3) / 8e12, 3))
    other = types.SimpleNamespace(grad=arena.grad.clone(), numel=arena.numel)

    def burst_alternating():
        for k in range(20):
            st["gn"].run(arena if k % 2 else other, start, mask, len(arena.params))
    d, h = measure(burst_alternating, 3, 10)
    row("3h the same burst alternating between two 448 MB arenas (no reuse out of the Infinity Cache)", d / 20, h / 20,
        TB_per_s=round(nbytes / (d / 20 * 1e-3) / 1e12, 3), fraction_of_8TBps=round(nbytes / (d / 20 * 1e-3) / 8e12, 3))
    del other
    keep = [g.clone() for g in grads]
    live = 0.9 * float(n3)   # after the first call the norm sits at max_norm: the coefficient stays just below 1
    d, h = measure(lambda: optim.clip_grad_norm_(model, live), a.warmup, a.reps)
    row("3b arena clip, live (norm pass + scale pass)", d, h, TB_per_s=round(3 * nbytes / (d * 1e-3) / 1e12, 3))
    torch._foreach_copy_(grads, keep)
    del keep

    # ---- the whole update, backward excluded
    def dummy_loss():
        return torch.zeros((), device=dev, requires_grad=True)

    def torch_op_scaler():
        s = torch.cuda.amp.GradScaler()

        def call(loss, optimizer, clip_grad=None, parameters=None, update_grad=True):
            s.scale(loss).backward()
            s.unscale_(optimizer)
            if clip_grad is not None:
                norm = torch.nn.utils.clip_grad_norm_(parameters, clip_grad)
            else:
                norm = misc._torch_grad_norm(list(parameters), 2.0)
            s.step(optimizer)
            s.update()
            return norm
        return call, s

    for clip in (None, 1e9):
        tag = "clip_grad=None" if clip is None else "clip_grad set"
        opt = optim.ArenaAdamW(model, param_groups(model), lr=1.5e-4, betas=(0.9, 0.95))
        call, s = torch_op_scaler()

        def rescale():   # what a scaled backward would have produced: unscale_ divides it out again
            torch._foreach_mul_(grads, s.get_scale())
        d_t, h_t = measure(lambda: call(dummy_loss(), opt, clip_grad=clip, parameters=model.parameters()),
                           a.warmup, a.reps, before=rescale)
        row(f"update, torch-op scaler + ArenaAdamW, {tag}", d_t, h_t)
        opt = optim.ArenaAdamW(model, param_groups(model), lr=1.5e-4, betas=(0.9, 0.95))
        native = misc.NativeScalerWithGradNormCount()
        d_n, h_n = measure(lambda: native(dummy_loss(), opt, clip_grad=clip, parameters=model.parameters()),
                           a.warmup, a.reps)
        row(f"update, native scaler + ArenaAdamW, {tag}", d_n, h_n,
            device_speedup=round(d_t / d_n, 2), host_speedup=round(h_t / h_n, 2))
        if clip is None:
            opt = optim.ArenaAdamW(model, param_groups(model), lr=1.5e-4, betas=(0.9, 0.95))
            d_p, h_p = measure(lambda: opt.step(), a.warmup, a.reps)
            row("plain ArenaAdamW.step(), for scale", d_p, h_p)
        del opt

    if a.log:
        with open(a.log, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
