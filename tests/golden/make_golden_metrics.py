"""Generator of tests/golden/g20_metrics.npz: the reference's OWN evaluation metrics run on the CPU.

    python tests/golden/make_golden_metrics.py [--ref /path/to/reference]

The two `Metrics/performance.py` files are imported by path (they import nothing but torch).  `rmse`, `rel_err`,
`abs_err` are the functions of `Depth_estimation/eval_depth.py`, imported as the module it is on top of
make_golden.py's torchvision restatement (it imports torchvision at module level), and `compute_scale_and_shift` is
the one of `Depth_estimation/Metrics/losses.py`.  Nothing is copied: the fixture holds inputs and recorded outputs only.

Contents:
  seg/{k}/logits, target, scores   k = 0..3: small logit and target maps [B, 1, H, W] and the reference's (Dice, IoU,
                                   precision, recall) on them; logits with |x| < 1e-3 are pushed out to +-1e-3, so the
                                   fp32 sigmoid band around 0 plays no part.  Case 3 is the all-empty one (Dice = 2.0).
  seg/nosig/...                    the same call with sigmoid=False on probabilities
  cls/{C}/preds, targets, scores   C = 6 and C = 23, predictions and targets with absent classes, and the reference's
                                   (mean F1, mean precision, mean recall)
  depth/{k}/pred, target, target_og, errors   k = 0..2: eval_depth.py:43-61 on one image each (scale_ = 10), the three
                                   errors.  torchvision is not installed here: TF.resize / TF.center_crop are
                                   F.interpolate(bilinear, align_corners=False) to max(h, w)^2 and a slice at
                                   torchvision's offsets int(round((M - h) / 2.0)).  That boundary stays unpinned,
                                   like row a14 of DESIGN.md section 4; everything else is the reference's code.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
from make_golden import _load_by_path, import_reference_models  # noqa: E402


def import_eval_depth():
    """the reference's eval_depth.py as a module: torchvision is the restatement, `Metrics` / `utils` resolve from the
    reference's own tree.  Its data loaders need torchvision.transforms, which the restatement does not have and the
    metric functions do not use: `Data.dataloaders` is an empty stand-in for the duration of the import."""
    import types
    import_reference_models()
    stand_in = {"Data": types.ModuleType("Data"), "Data.dataloaders": types.ModuleType("Data.dataloaders")}
    stand_in["Data"].dataloaders = stand_in["Data.dataloaders"]
    saved = {k: sys.modules.get(k) for k in stand_in}
    sys.modules.update(stand_in)
    app = os.path.join(mg.REF, "Depth_estimation")
    for p in (mg.REF, app):
        if p not in sys.path:
            sys.path.insert(0, p)
    cwd = os.getcwd()
    os.chdir(app)  # eval_depth.py reaches utils.py through sys.path.append("..")
    try:
        return _load_by_path("ref_eval_depth", os.path.join(app, "eval_depth.py"))
    finally:
        os.chdir(cwd)
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def push_out(x, eps=1e-3):
    return torch.where(x.abs() < eps, torch.where(x < 0, -eps, eps).to(x.dtype), x)


def seg_cases(perf, out):
    g = torch.Generator("cpu").manual_seed(201)
    fns = (perf.DiceScore(), perf.IoU(), perf.Precision(), perf.Recall())
    shapes = ((3, 1, 7, 5), (1, 1, 16, 16), (2, 1, 33, 40))
    for k, shp in enumerate(shapes):
        logits = push_out(3.0 * torch.randn(shp, generator=g))
        target = (torch.rand(shp, generator=g) < 0.4).float()
        if k == 0:
            logits[1] = -logits[1].abs()   # an all-negative image: empty prediction
            logits[2] = logits[2].abs()    # an all-positive one
        out[f"seg/{k}/logits"], out[f"seg/{k}/target"] = logits.numpy(), target.numpy()
        out[f"seg/{k}/scores"] = np.array([float(f(logits, target)) for f in fns], dtype=np.float32)
    logits = -push_out(torch.randn(2, 1, 8, 8, generator=g)).abs()
    target = torch.zeros(2, 1, 8, 8)
    out["seg/3/logits"], out["seg/3/target"] = logits.numpy(), target.numpy()
    out["seg/3/scores"] = np.array([float(f(logits, target)) for f in fns], dtype=np.float32)
    assert out["seg/3/scores"].tolist() == [2.0, 1.0, 1.0, 1.0], out["seg/3/scores"]
    probs = torch.rand(2, 1, 9, 11, generator=g)
    target = (torch.rand(2, 1, 9, 11, generator=g) < 0.5).float()
    out["seg/nosig/logits"], out["seg/nosig/target"] = probs.numpy(), target.numpy()
    out["seg/nosig/scores"] = np.array([float(f(probs, target, sigmoid=False)) for f in fns], dtype=np.float32)
    print("g20 seg:", {k: out[f"seg/{k}/scores"].tolist() for k in (0, 1, 2, 3, "nosig")}, flush=True)


def cls_cases(perf, out):
    g = torch.Generator("cpu").manual_seed(202)
    for C, n, absent in ((6, 97, (4, 5)), (23, 640, (0, 7, 22))):
        present = torch.tensor([c for c in range(C) if c not in absent])
        targets = present[torch.randint(0, len(present), (n,), generator=g)]
        preds = torch.where(torch.rand(n, generator=g) < 0.7, targets,
                            present[torch.randint(0, len(present), (n,), generator=g)])
        preds[:3] = absent[0] if C == 6 else preds[:3]  # C = 6: class 4 is predicted but never a target, class 5 is absent from both
        fns = (perf.meanF1Score(C), perf.meanPrecision(C), perf.meanRecall(C))
        out[f"cls/{C}/preds"], out[f"cls/{C}/targets"] = preds.numpy(), targets.numpy()
        out[f"cls/{C}/scores"] = np.array([float(f(preds, targets)) for f in fns], dtype=np.float32)
        print(f"g20 cls C={C}:", out[f"cls/{C}/scores"].tolist(), flush=True)


def depth_cases(ev, ref_losses, out):
    g = torch.Generator("cpu").manual_seed(203)
    scale_ = 10
    for k, (S, h, w) in enumerate(((16, 23, 29), (16, 29, 22), (32, 40, 40))):
        target = torch.rand(1, S, S, generator=g)
        target = torch.where(torch.rand(1, S, S, generator=g) < 0.25, torch.zeros(()), target)
        output = 0.6 * target + 0.1 + 0.05 * torch.randn(1, S, S, generator=g)
        target_og = torch.rand(1, 1, h, w, generator=g)
        target_og = torch.where(torch.rand(1, 1, h, w, generator=g) < 0.25, torch.zeros(()), target_og)
        out[f"depth/{k}/pred"], out[f"depth/{k}/target"] = output.numpy().copy(), target.numpy().copy()
        out[f"depth/{k}/target_og"] = target_og.numpy().copy()
        # eval_depth.py:43-61; the two torchvision calls as torch ops (see the module docstring)
        scale, shift = ref_losses.compute_scale_and_shift(output, target, target > 0.0)
        output = scale.view(-1, 1, 1) * output + shift.view(-1, 1, 1)
        max_size = max(h, w)
        output = F.interpolate(output.unsqueeze(1), size=(max_size, max_size), mode="bilinear", align_corners=False)
        top, left = int(round((max_size - h) / 2.0)), int(round((max_size - w) / 2.0))
        output = output[..., top:top + h, left:left + w]
        output[output < 0.0] = 0.0
        output[output > 1.0] = 1.0
        output[target_og == 0.0] = 0.0
        output *= scale_
        target_og *= scale_
        out[f"depth/{k}/errors"] = np.array([ev.rmse(output, target_og), ev.rel_err(output, target_og),
                                             ev.abs_err(output, target_og)], dtype=np.float32)
        print(f"g20 depth {k} (S={S}, {h}x{w}):", out[f"depth/{k}/errors"].tolist(), flush=True)
    out["depth/scale_"] = np.array(float(scale_))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=None, help="root of the reference checkout (default: make_golden.py's)")
    a = ap.parse_args()
    if a.ref:
        mg.REF = os.path.abspath(a.ref)
    seg_perf = _load_by_path("ref_seg_performance", os.path.join(mg.REF, "Binary_segmentation", "Metrics", "performance.py"))
    cls_perf = _load_by_path("ref_cls_performance", os.path.join(mg.REF, "Classification", "Metrics", "performance.py"))
    ref_losses = _load_by_path("ref_depth_losses", os.path.join(mg.REF, "Depth_estimation", "Metrics", "losses.py"))
    ev = import_eval_depth()
    out = {}
    seg_cases(seg_perf, out)
    cls_cases(cls_perf, out)
    depth_cases(ev, ref_losses, out)
    path = os.path.join(HERE, "g20_metrics.npz")
    np.savez_compressed(path, **out)
    print(f"g20 ok: {os.path.getsize(path) / 1024:.0f} KiB")
    assert os.path.getsize(path) < 512 * 1024


if __name__ == "__main__":
    main()
