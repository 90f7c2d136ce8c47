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

    python tools/pack_images.py /data/kvasir-seg/images --ragged --boxes /data/kvasir-seg/bounding-boxes.json --out kvasir_det
      -> kvasir_det.pixels.npy       [total] uint8: every image at its OWN size, HWC rows dense, each starting at a
                                     multiple of 16 bytes (ssl4gie_amd.data.RaggedImageBank.from_npy loads the four)
         kvasir_det.sizes.npy        [n, 2] int32 (H, W)
         kvasir_det.boxes.npy        [m, 4] float32 (xmin, ymin, xmax, ymax) in stored-image pixels, from Kvasir's JSON
                                     ({name: {"bbox": [{"xmin": ..}, ..]}}, read as Object_detection/train_detection.py:154-166)
         kvasir_det.box_offsets.npy  [n + 1] int64: image k owns rows box_offsets[k] .. box_offsets[k + 1]
         kvasir_det.files.txt        the file names in bank order: sorted(glob), as train_detection.py:172-173

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


def pack_ragged(root, boxes_json, out, limit=None):
    """every image of a flat folder at its own size + Kvasir's boxes -> the four files of a RaggedImageBank"""
    import json
    names = sorted(f for f in os.listdir(root) if f.lower().endswith(EXTENSIONS))[:limit]   # sorted(glob(root + "*"))
    if not names:
        raise SystemExit(f"no images under {root}")
    with open(boxes_json) as f:
        table = json.load(f)
    sizes = np.zeros((len(names), 2), np.int32)
    for k, name in enumerate(names):
        with Image.open(os.path.join(root, name)) as im:
            sizes[k] = (im.size[1], im.size[0])
    if sizes.min() < 13:
        raise SystemExit("an image has a side below 13 pixels: the 25-tap blur reflects 12")
    nbytes = (sizes[:, 0].astype(np.int64) * sizes[:, 1] * 3 + 15) // 16 * 16
    ends = np.cumsum(nbytes)
    flat = np.lib.format.open_memmap(out + ".pixels.npy", mode="w+", dtype=np.uint8, shape=(int(ends[-1]),))
    boxes, offsets = [], [0]
    for k, name in enumerate(names):
        with Image.open(os.path.join(root, name)) as im:
            a = np.asarray(im.convert("RGB"), dtype=np.uint8)
        start = int(ends[k] - nbytes[k])
        flat[start:start + a.size] = a.reshape(-1)
        flat[start + a.size:int(ends[k])] = 0
        entry = table.get(os.path.splitext(name)[0], table.get(name))
        if entry is None:
            raise SystemExit(f"{name}: no entry in {boxes_json}")
        boxes += [[b["xmin"], b["ymin"], b["xmax"], b["ymax"]] for b in entry["bbox"]]
        offsets.append(len(boxes))
    flat.flush()
    del flat
    np.save(out + ".sizes.npy", sizes)
    np.save(out + ".boxes.npy", np.asarray(boxes, dtype=np.float32).reshape(-1, 4))
    np.save(out + ".box_offsets.npy", np.asarray(offsets, dtype=np.int64))
    with open(out + ".files.txt", "w") as f:
        f.writelines(n + "\n" for n in names)
    return len(names), len(boxes), int(ends[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("root")
    ap.add_argument("--out", required=True, help="output prefix")
    ap.add_argument("--size", type=int, nargs="+", default=[256], help="stored size: S, or H W")
    ap.add_argument("--center-crop", action="store_true")
    ap.add_argument("--limit", type=int, default=None)
    ap.add_argument("--targets", default=None, help="folder of masks (8-bit) or depth maps (16-bit), one per image")
    ap.add_argument("--ragged", action="store_true", help="keep every image at its own size (detection): needs --boxes")
    ap.add_argument("--boxes", default=None, help="Kvasir's bounding-boxes.json, with --ragged")
    a = ap.parse_args()
    if a.ragged or a.boxes:
        if not (a.ragged and a.boxes):
            raise SystemExit("--ragged and --boxes come together")
        n, m, total = pack_ragged(a.root, a.boxes, a.out, a.limit)
        print(f"{n} images, {m} boxes -> {a.out}.pixels.npy [{total}] uint8 ({total / 1e9:.2f} GB), .sizes.npy, .boxes.npy, "
              f".box_offsets.npy")
        return
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
