"""Generator of tests/golden/g21_det_loader.npz: the reference's OWN detection dataset class run on the CPU.

    python tests/golden/make_golden_det_loader.py [--ref /path/to/reference]

`Object_detection/Data/dataset.py` is imported by path and its `Dataset.__getitem__` is run on small PNGs written to a
temporary folder (rotate, hflip and vflip on, arch != "resnet50", fixed_size = 64).  Nothing is copied: the fixture
holds inputs and recorded outputs only.

torchvision is not installed here.  For the duration of the import a stand-in `torchvision.transforms`
(`InterpolationMode`) and `torchvision.transforms.functional` (`hflip`, `vflip`, `pad`, `resize`) made of torch ops is
registered: flip(-1), flip(-2), F.pad with zeros, and F.interpolate(mode="bicubic", antialias=True,
align_corners=False) — what torchvision's tensor path calls.  The resize therefore stays unpinned at the torchvision
boundary, like row a14 of DESIGN.md section 4 and G20; everything else is the reference's code.  `transform_input` is
ToTensor's statement, uint8 -> float -> .div(255).  `random.uniform` is wrapped while an item is fetched: it hands out
a scripted value above or below 0.5 and records the three decisions.

Contents, case k = 0 .. 13:
  img/{k}        uint8 [H, W, 3], the stored image            boxes/{k}      fp32 [n, 4] (xmin, ymin, xmax, ymax), n in {0, 1, 3}
  dec/{k}        uint8 [3] = (rotate, hflip, vflip)            out_img/{k}    fp32 [3, 64, 64], what __getitem__ returned
  out_boxes/{k}  fp32 [n, 4]
  fixed_size     64
Cases: 71 x 93 (both sides odd, halved, unequal pads 8 / 9) under all eight decisions; 40 x 56 (no halving), 64 x 64
(exact fit), 100 x 50 (only H exceeds), 65 x 20 (odd H exceeds, even W), 128 x 128 (halves to an exact fit) and 13 x 13
(the smallest side) under one combination each.
"""
from __future__ import annotations

import argparse
import os
import random
import sys
import tempfile
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
from make_golden import _load_by_path  # noqa: E402

FIXED = 64
# (H, W, (rotate, hflip, vflip), boxes)
CASES = [(71, 93, (r, h, v), (3, 1, 0)[(4 * r + 2 * h + v) % 3]) for r in (0, 1) for h in (0, 1) for v in (0, 1)] + [
    (40, 56, (1, 0, 1), 3), (64, 64, (0, 1, 0), 1), (100, 50, (0, 1, 1), 3), (65, 20, (0, 0, 1), 1),
    (128, 128, (1, 1, 0), 3), (13, 13, (1, 1, 1), 0)]


def import_reference_dataset():
    """the reference's Data/dataset.py on top of a torch-op stand-in for the four torchvision calls it makes"""
    tv, tr, tf = (types.ModuleType(n) for n in ("torchvision", "torchvision.transforms", "torchvision.transforms.functional"))

    class InterpolationMode:
        BICUBIC = "bicubic"

    def pad(x, padding):                     # torchvision's (left, top, right, bottom), constant 0
        left, top, right, bottom = padding
        return F.pad(x, (left, right, top, bottom))

    def resize(x, size, interpolation, antialias):
        assert interpolation == InterpolationMode.BICUBIC and antialias
        return F.interpolate(x.unsqueeze(0), size=tuple(size), mode="bicubic", antialias=True, align_corners=False).squeeze(0)

    tr.InterpolationMode = InterpolationMode
    tf.hflip, tf.vflip, tf.pad, tf.resize = (lambda x: x.flip(-1)), (lambda x: x.flip(-2)), pad, resize
    tv.transforms, tr.functional = tr, tf
    stand_in = {m.__name__: m for m in (tv, tr, tf)}
    saved = {k: sys.modules.get(k) for k in stand_in}
    sys.modules.update(stand_in)
    try:
        return _load_by_path("ref_det_dataset", os.path.join(mg.REF, "Object_detection", "Data", "dataset.py"))
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def to_tensor(pil):
    """transforms.ToTensor on an 8-bit RGB image"""
    return torch.from_numpy(np.asarray(pil, dtype=np.uint8).copy()).permute(2, 0, 1).contiguous().to(torch.float32).div(255)


def make_image(rng, H, W):
    """noise on a smooth ramp: every pixel differs from its neighbours, and a misplaced pixel shows"""
    y, x = np.meshgrid(np.arange(H) / H, np.arange(W) / W, indexing="ij")
    base = np.stack([200 * x, 200 * y, 100 + 100 * (x - y)], axis=2)
    return np.clip(base + rng.integers(0, 56, size=(H, W, 3)), 0, 255).astype(np.uint8)


def make_boxes(rng, H, W, n):
    b = np.zeros((n, 4), np.float32)
    for i in range(n):
        x = np.sort(rng.uniform(0, W, 2))
        y = np.sort(rng.uniform(0, H, 2))
        b[i] = (x[0], y[0], x[1], y[1])
    return b


def main():
    from PIL import Image
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=None, help="root of the reference checkout (default: make_golden.py's)")
    a = ap.parse_args()
    if a.ref:
        mg.REF = os.path.abspath(a.ref)
    ref = import_reference_dataset()
    rng = np.random.default_rng(2100)
    out = {"fixed_size": np.array(FIXED)}
    real_uniform = random.uniform
    with tempfile.TemporaryDirectory() as tmp:
        paths, targets = [], {}
        for k, (H, W, _, n) in enumerate(CASES):
            img = make_image(rng, H, W)
            path = os.path.join(tmp, f"{k:02d}.png")
            Image.fromarray(img).save(path)
            paths.append(path)
            targets[path] = make_boxes(rng, H, W, n)
            out[f"img/{k}"], out[f"boxes/{k}"] = img, targets[path]

        def target_vals(input_id, tg):   # train_detection.py:154-166: one class, label 1
            b = torch.from_numpy(tg[input_id].copy())
            return {"boxes": b, "labels": torch.ones(len(b), dtype=torch.int64)}

        ds = ref.Dataset(paths, targets, target_vals, transform_input=to_tensor, hflip=True, vflip=True, rotate=True,
                         arch="vit-b", fixed_size=FIXED)
        for k, (H, W, dec, n) in enumerate(CASES):
            script, seen = list(dec), []

            def uniform(lo, hi):
                u = 0.75 if script.pop(0) else 0.25
                seen.append(u > 0.5)
                return lo + (hi - lo) * u

            random.uniform = uniform
            try:
                x, t = ds[k]
            finally:
                random.uniform = real_uniform
            assert len(seen) == 3 and not script and tuple(x.shape) == (3, FIXED, FIXED) and x.dtype == torch.float32
            out[f"dec/{k}"] = np.array(seen, dtype=np.uint8)
            out[f"out_img/{k}"], out[f"out_boxes/{k}"] = x.numpy().copy(), t["boxes"].numpy().copy().reshape(-1, 4)
            print(f"g21 case {k}: {H} x {W}, (r, h, v) = {dec}, {n} boxes -> {out[f'out_boxes/{k}'].tolist()}", flush=True)
    path = os.path.join(HERE, "g21_det_loader.npz")
    np.savez_compressed(path, **out)
    print(f"g21 ok: {os.path.getsize(path) / 1024:.0f} KiB")
    assert os.path.getsize(path) < 1024 * 1024


if __name__ == "__main__":
    main()
