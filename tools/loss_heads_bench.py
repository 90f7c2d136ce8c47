#!/usr/bin/env python3
"""Loss sections alone, torch-op path against the fused kernels of csrc/loss_ops.hip, in one process:

    InfoNCE          (256, 2048, 256), forward + backward       MoCo.contrastive_loss, SSL4GIE_FUSED_INFONCE 0 / 1
    cross-entropy    (256, 12), forward + backward              nn.CrossEntropyLoss(weight) / losses.CrossEntropyLoss
    Barlow Twins     D = 8192, bf16 operands                    cross_corr_loss_terms + dc * s + cast + cast_transpose
                                                                / ssl4gie_bt_loss + ssl4gie_bt_loss_grad

usage: loss_heads_bench.py [--reps 200] [--warmup 20]      device events around `reps` repetitions, the two paths
                                                           alternating (torch, fused, torch, fused); prints ms per
                                                           repetition and the Barlow Twins kernels' bytes/s
       loss_heads_bench.py --trace                         ONE repetition of every (section, path) after a warm-up,
                                                           each bracketed by a marker kernel: run it under
                                                           `rocprofv3 --kernel-trace --output-format csv`
       loss_heads_bench.py --count kernel_trace.csv        launches per (section, path) from that trace
"""
import argparse
import csv
import os
import sys
from types import SimpleNamespace

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

MARK = "random_"  # the marker launch: Tensor.random_() is used nowhere in the sections


def sections():
    import torch
    import torch.nn as nn
    from ssl4gie_amd import ops
    from ssl4gie_amd.losses import CrossEntropyLoss
    from ssl4gie_amd.Models.barlow_twins import cross_corr_loss_terms
    from ssl4gie_amd.Models.moco_v3.moco.builder import MoCo
    dev = "cuda"
    g = torch.Generator("cpu").manual_seed(0)
    q = torch.randn(256, 256, generator=g).to(dev).requires_grad_(True)
    k = torch.randn(2048, 256, generator=g).to(dev)
    me = SimpleNamespace(T=0.2)

    def nce(fused):
        os.environ["SSL4GIE_FUSED_INFONCE"] = "1" if fused else "0"
        q.grad = None
        # the keys of one rank stand in for the gathered ones: world = 1 here, the shapes are the 8-rank ones
        MoCo.contrastive_loss(me, q, k).backward()

    x = torch.randn(256, 12, generator=g).to(dev).requires_grad_(True)
    t = torch.randint(0, 12, (256,), generator=g).to(dev)
    w = (torch.rand(12, generator=g) + 0.1).to(dev)
    ce_t, ce_f = nn.CrossEntropyLoss(w), CrossEntropyLoss(w).to(dev)

    def ce(fused):
        x.grad = None
        (ce_f if fused else ce_t)(x, t).backward()

    D, lambd, n_global = 8192, 0.0051, 2048
    c = (0.05 * torch.randn(D, D, generator=g) + 0.9 * torch.eye(D)).to(dev)
    gout = torch.ones((), device=dev)

    def bt(fused):
        if fused:
            loss = ops.bt_loss(c, lambd)
            wv, wt = ops.bt_loss_grad(c, gout / n_global, torch.bfloat16, lambd)
        else:
            loss, dc = cross_corr_loss_terms(c, lambd)
            dc = dc * (gout / n_global)
            wv, wt = ops.cast(dc, torch.bfloat16), ops.cast_transpose(dc, torch.bfloat16)
        return loss, wv, wt

    def bt_kernels():  # the two fused kernels one by one, for the bytes/s figures
        s = gout / n_global
        return (lambda: ops.bt_loss(c, lambd)), (lambda: ops.bt_loss_grad(c, s, torch.bfloat16, lambd)), D

    return [("infonce_256x2048x256_fwd_bwd", nce), ("cross_entropy_256x12_fwd_bwd", ce), ("bt_terms_8192_bf16", bt)], \
        bt_kernels


def timed(fn, reps):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def count(path):
    rows = list(csv.DictReader(open(path)))
    key = next(k for k in rows[0] if k.lower() in ("kernel_name", "kernelname", "name"))
    start = next(k for k in rows[0] if k.lower() in ("start_timestamp", "beginns", "start"))
    rows.sort(key=lambda r: int(r[start]))
    names = [r[key] for r in rows]
    marks = [i for i, n in enumerate(names) if MARK in n]
    labels = [f"{s} {p}" for s in ("infonce", "cross_entropy", "bt_terms") for p in ("torch", "fused")]
    assert len(marks) == len(labels) + 1, (len(marks), "marker launches found")
    for lab, lo, hi in zip(labels, marks[:-1], marks[1:]):
        print(f"{lab:28s} {hi - lo - 1:4d} launches")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--count", default=None)
    a = ap.parse_args()
    if a.count:
        return count(a.count)
    import torch
    secs, bt_kernels = sections()
    for _, fn in secs:
        for _ in range(a.warmup):
            fn(False)
            fn(True)
    torch.cuda.synchronize()
    if a.trace:
        mark = torch.empty(64, device="cuda")
        for _, fn in secs:
            for fused in (False, True):
                mark.random_()
                fn(fused)
        mark.random_()
        torch.cuda.synchronize()
        return
    for name, fn in secs:
        ms = [timed(lambda: fn(f), a.reps) for f in (False, True, False, True)]
        print(f"{name:32s} torch {ms[0] * 1e3:8.1f} / {ms[2] * 1e3:8.1f} us   fused {ms[1] * 1e3:8.1f} / "
              f"{ms[3] * 1e3:8.1f} us   ({a.reps} repetitions each, alternating)")
    loss_fn, grad_fn, D = bt_kernels()
    for _ in range(a.warmup):
        loss_fn(), grad_fn()
    t_loss, t_grad = timed(loss_fn, a.reps), timed(grad_fn, a.reps)
    b_loss, b_grad = 4.0 * D * D, (4.0 + 2.0 + 2.0) * D * D  # algorithmic bytes: one fp32 read; one read, two bf16 writes
    print(f"ssl4gie_bt_loss      D={D}: {t_loss * 1e3:8.1f} us  {b_loss / t_loss / 1e9:6.2f} TB/s of the 8 TB/s roof")
    print(f"ssl4gie_bt_loss_grad D={D}: {t_grad * 1e3:8.1f} us  {b_grad / t_grad / 1e9:6.2f} TB/s of the 8 TB/s roof")


if __name__ == "__main__":
    main()
