#!/usr/bin/env python
"""Pack an image folder into the uint8 bank that ssl4gie_amd.data.DeviceImageBank.from_npy loads: host-side, PIL,
run once per dataset.

    python tools/pack_images.py /data/hyperkvasir/unlabelled --out train_256 --size 256
      -> train_256.npy          [n, 256, 256, 3] uint8 (written through a memory map: one image in memory at a time)
         train_256.labels.npy   [n] int64: index of the image's top-level sub-folder, sorted by name (ImageFolder's
                                class_to_idx); all 0 for a flat folder
         train_256.files.txt    the relative paths, in bank order

    python tools/pack_images.py /data/kvasir-seg/images --targets /data/kvasir-seg/masks --out train_224 --size 224
      -> also train_224.targets.npy  [n, 224, 224] uint8 (masks, any 8-bit mode, taken to "L") or uint16 (16-bit depth
                                     maps), file k of the targets folder (same order rule) beside image k: the
                                     `targets=` of DeviceImageBank.from_npy, for ssl4gie_amd.data.FinetuneAugment

Every image is converted to RGB and resized to the stored size (--size S: S x S; --size H W) with PIL's antialiased
bicubic filter, aspect ratio NOT preserved unless --center-crop first cuts the largest centred region of the
target's aspect.  The stored size is what the random crops are later taken from: 256 for a 224 training size keeps
the bank of a ~100 k-image dataset under 20 GB.  Targets are resized with PIL's default filter for Image.resize, as
the reference's finetune datasets resize them when they load a file (Binary_segmentation/Data/dataset.py:41,
Depth_estimation/Data/dataset.py:49): bicubic for 8-bit modes, nearest for 16-bit ones."""
import argparse
import os

import numpy as np
from PIL import Image

EXTENSIONS = (".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".pgm", ".tif", ".tiff", ".webp")


def find_images(root):
    """(relative path, label) in ImageFolder's order: classes sorted, then walk order within a class"""
    root = os.path.abspath(root)
    classes = sorted(d.name for d in os.scandir(root) if d.is_dir())
    items = []
    for label, cls in enumerate(classes):
        for base, _, files in sorted(os.walk(os.path.join(root, cls), followlinks=True)):
            items += [(os.path.relpath(os.path.join(base, f), root), label) for f in sorted(files)
                      if f.lower().endswith(EXTENSIONS)]
    if not items:   # a flat folder
        items = [(f, 0) for f in sorted(os.listdir(root)) if f.lower().endswith(EXTENSIONS)]
    return items


def load_resized(path, Hs, Ws, center_crop):
    with Image.open(path) as im:
        im = im.convert("RGB")
        if center_crop:
            w, h = im.size
            cw = min(w, int(round(h * Ws / Hs)))
            ch = min(h, int(round(w * Hs / Ws)))
            left, top = (w - cw) // 2, (h - ch) // 2
            im = im.crop((left, top, left + cw, top + ch))
        if im.size != (Ws, Hs):
            im = im.resize((Ws, Hs), Image.BICUBIC)
        return np.asarray(im, dtype=np.uint8)


def load_target(path, Hs, Ws):
    """uint16 [Hs, Ws] for a 16-bit image, else uint8 (mode "L")"""
    with Image.open(path) as im:
        deep = im.mode.startswith("I")                     # I;16 and its kin, I
        if im.size != (Ws, Hs):
            im = im.resize((Ws, Hs))                       # PIL's default filter for the mode
        return np.asarray(im).astype(np.uint16) if deep else np.asarray(im.convert("L"), dtype=np.uint8)


def pack_targets(root, out, Hs, Ws, n, limit=None):
    """the targets folder, in find_images' order, to out.targets.npy; there must be one per image"""
    items = find_images(root)[:limit]
    if len(items) != n:
        raise SystemExit(f"{len(items)} targets under {root} for {n} images")
    first = load_target(os.path.join(root, items[0][0]), Hs, Ws)
    bank = np.lib.format.open_memmap(out + ".targets.npy", mode="w+", dtype=first.dtype, shape=(n, Hs, Ws))
    for k, (rel, _) in enumerate(items):
        t = load_target(os.path.join(root, rel), Hs, Ws)
        if t.dtype != first.dtype:
            raise SystemExit(f"{rel}: {t.dtype} among {first.dtype} targets")
        bank[k] = t
    bank.flush()
    return first.dtype


def pack(root, out, Hs, Ws, center_crop=False, limit=None):
    items = find_images(root)[:limit]
    if not items:
        raise SystemExit(f"no images under {root}")
    bank = np.lib.format.open_memmap(out + ".npy", mode="w+", dtype=np.uint8, shape=(len(items), Hs, Ws, 3))
    for k, (rel, _) in enumerate(items):
        bank[k] = load_resized(os.path.join(root, rel), Hs, Ws, center_crop)
    bank.flush()
    del bank
    np.save(out + ".labels.npy", np.asarray([label for _, label in items], dtype=np.int64))
    with open(out + ".files.txt", "w") as f:
        f.writelines(rel + "\n" for rel, _ in items)
    return len(items)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("root")
    ap.add_argument("--out", required=True, help="output prefix")
    ap.add_argument("--size", type=int, nargs="+", default=[256], help="stored size: S, or H W")
    ap.add_argument("--center-crop", action="store_true")
    ap.add_argument("--limit", type=int, default=None)
    ap.add_argument("--targets", default=None, help="folder of masks (8-bit) or depth maps (16-bit), one per image")
    a = ap.parse_args()
    Hs, Ws = (a.size[0], a.size[0]) if len(a.size) == 1 else (a.size[0], a.size[1])
    if a.targets and a.center_crop:
        raise SystemExit("--targets with --center-crop is not supported: the reference squashes both to the size")
    n = pack(a.root, a.out, Hs, Ws, a.center_crop, a.limit)
    print(f"{n} images -> {a.out}.npy [{n}, {Hs}, {Ws}, 3] uint8 ({n * Hs * Ws * 3 / 1e9:.2f} GB)")
    if a.targets:
        dtype = pack_targets(a.targets, a.out, Hs, Ws, n, a.limit)
        print(f"{n} targets -> {a.out}.targets.npy [{n}, {Hs}, {Ws}] {dtype}")


if __name__ == "__main__":
    main()
