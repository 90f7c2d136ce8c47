"""Generator of tests/golden/g22_linprobe.npz: the MAE linear probe's head trained by the reference's OWN LARS.

    python tests/golden/make_golden_linprobe.py --ref /path/to/reference

`Models/mae/util/lars.py` is imported by path (it imports nothing but torch).  The head is the one
`Models/mae/main_linprobe.py:222` builds, `Sequential(BatchNorm1d(192, affine=False, eps=1e-6), Linear(192, 10))`,
stepped 5 times at batch 16 with `CrossEntropyLoss` and `LARS(head.parameters(), lr=6.4, weight_decay=1e-3)` —
the recipe's rate (blr 0.1 x 16384 / 256): LARS moves a matrix by lr x trust_coefficient = 0.64 % of its norm per
step, so five steps move the weight by several per cent, far above the 1e-3 bar it is held to.  Nothing is copied: the
fixture holds inputs and recorded outputs only.

Inputs come from oracle.synth's keyed generator: features [5, 16, 192] with a per-feature offset and scale (so that the
BatchNorm has something to do), ROUNDED TO bf16-REPRESENTABLE VALUES — the engine hands its head features in the
operand type, and both arithmetics then start from the same numbers —, targets [5, 16], the initial weight (0.01 x a
clipped normal, main_linprobe.py:218) and a zero bias.

Contents:
  x, target, weight0, bias0, lr, weight_decay, momentum, trust_coefficient
  fp32/{loss, weight, bias, running_mean, running_var}   per step [5, ...], the reference in fp32
  fp64/{...}                                              the same run in double
  bf16_err/{...}                                          [5] per quantity: relative L2 error of the reference's own
                                                          torch.autocast("cpu", bfloat16) run against the double run
  fp32_err/{...}                                          the same for the fp32 run (information)
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import synth  # noqa: E402

D, C, B, STEPS, SEED = 192, 10, 16, 5, 22
LR, WD, MOM, TRUST = 6.4, 1e-3, 0.9, 0.001
NAMES = ("loss", "weight", "bias", "running_mean", "running_var")


def load_lars(ref):
    spec = importlib.util.spec_from_file_location("ref_lars", os.path.join(ref, "Models", "mae", "util", "lars.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.LARS


def inputs():
    g = synth._gen("g22/linprobe", SEED)
    offset, scale = torch.randn(D, generator=g), 0.5 + 1.5 * torch.rand(D, generator=g)
    x = (torch.randn(STEPS, B, D, generator=g) * scale + offset).bfloat16().float()
    target = torch.randint(0, C, (STEPS, B), generator=g)
    w0 = 0.01 * torch.randn(C, D, generator=g).clamp(-2.0, 2.0)
    return x, target, w0, torch.zeros(C)


def run(LARS, x, target, w0, b0, mode):
    dt = torch.float64 if mode == "fp64" else torch.float32
    head = torch.nn.Sequential(torch.nn.BatchNorm1d(D, affine=False, eps=1e-6), torch.nn.Linear(D, C)).to(dt)
    with torch.no_grad():
        head[1].weight.copy_(w0)
        head[1].bias.copy_(b0)
    head.train()
    opt = LARS(head.parameters(), lr=LR, weight_decay=WD, momentum=MOM, trust_coefficient=TRUST)
    crit = torch.nn.CrossEntropyLoss()
    out = {k: [] for k in NAMES}
    for s in range(STEPS):
        if mode == "bf16":
            with torch.autocast("cpu", dtype=torch.bfloat16):
                logits = head(x[s])
            loss = crit(logits.float(), target[s])
        else:
            loss = crit(head(x[s].to(dt)), target[s])
        opt.zero_grad()
        loss.backward()
        opt.step()
        out["loss"].append(loss.detach().double().reshape(1))
        out["weight"].append(head[1].weight.detach().double().clone())
        out["bias"].append(head[1].bias.detach().double().clone())
        out["running_mean"].append(head[0].running_mean.detach().double().clone())
        out["running_var"].append(head[0].running_var.detach().double().clone())
    return {k: torch.stack(v) for k, v in out.items()}


def l2_err(a, b):
    return [float((a[s] - b[s]).norm() / b[s].norm()) for s in range(a.shape[0])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="root of the reference tree")
    args = ap.parse_args()
    LARS = load_lars(args.ref)
    torch.manual_seed(0)
    x, target, w0, b0 = inputs()
    runs = {m: run(LARS, x, target, w0, b0, m) for m in ("fp64", "fp32", "bf16")}
    out = {"x": x.numpy(), "target": target.numpy(), "weight0": w0.numpy(), "bias0": b0.numpy(),
           "lr": np.array(LR), "weight_decay": np.array(WD), "momentum": np.array(MOM),
           "trust_coefficient": np.array(TRUST)}
    for k in NAMES:
        out[f"fp64/{k}"] = runs["fp64"][k].numpy()
        out[f"fp32/{k}"] = runs["fp32"][k].float().numpy()
        out[f"bf16_err/{k}"] = np.array(l2_err(runs["bf16"][k], runs["fp64"][k]))
        out[f"fp32_err/{k}"] = np.array(l2_err(runs["fp32"][k], runs["fp64"][k]))
        print(f"g22 {k}: fp32 err {max(out[f'fp32_err/{k}']):.3e}  bf16-autocast err per step "
              + " ".join(f"{e:.3e}" for e in out[f"bf16_err/{k}"]))
    moved = float((runs["fp64"]["weight"][-1] - w0.double()).norm() / w0.double().norm())
    print(f"g22: loss {runs['fp64']['loss'].flatten().tolist()}  weight moved by {moved:.3f} of its norm")
    np.savez_compressed(os.path.join(HERE, "g22_linprobe.npz"), **out)
    print("g22 ok")


if __name__ == "__main__":
    main()
